/*
 * atrac1_oracle_f32.c -- the oracle with every `double` read as `float`: a binary32 twin of its decoder.
 *
 * TEST INFRASTRUCTURE ONLY, like the oracle itself.  It answers one question: what does binary32 arithmetic cost
 * this decoder, in the reference's own operation order (radix-2, tables rounded to binary32 when they are read)?
 * It is the yardstick of tests/decode32_lib.py, not a model of k_decode<float>.
 *
 * Only c1o_pack_unit, c1o_unpack_unit, c1o_decode_frame and c1o_decode_stream keep their ABI under the define:
 * their arguments hold no double.  Bind and use nothing else from this library (c1o_options, c1o_set_tables,
 * c1o_allocate, c1o_libm, ... all change shape, and the encoder side in binary32 is nobody's reference).
 *
 * The system headers come first so that their own prototypes are declared with the real double.
 */
#include <stdint.h>
#include <math.h>
#include <string.h>

#define double float
#include "atrac1_oracle.c"
