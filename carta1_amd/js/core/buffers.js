// BufferPool: in the reference (codec/core/buffers.js:7-81) this object IS the per-stream codec state
// (QMF delay lines, MDCT overlap, transient history, IMDCT tails).  Here that state lives on the GPU
// inside a native stream handle; the pool owns the handle so that, exactly as in the reference, passing
// the same pool to encode()/decode() continues the same stream and a fresh pool starts a new one.
//
// The state can leave and enter the pool in the reference's own layout: getEncoderState() / getDecoderState() return the
// typed arrays the reference's pool would hold after the same calls, setEncoderState(obj) / setDecoderState(obj) take any
// object with those fields -- an instance of the reference's own BufferPool qualifies -- and the encode() / decode()
// closures of this pool continue from it (c1_enc_stream_get_state and its kin, include/carta1_hip.h).  A set on a pool whose
// native stream does not exist yet is kept and applied when the first closure call creates it.  Only the closures' streams
// are concerned: the separate histories of the single-stage exports below (qmfHistory, transientBands, mdctPreviousBands,
// imdctPrevious, synthesisPreviousBands) are not touched.
import { native } from '../native.js'

const QMF_DELAY = 46
const QMF_HIGH_BAND_DELAY = 39
const MDCT_OVERLAP = [32, 32, 32]
const TRANSIENT_BINS = [64, 64, 128]
const IMDCT_OVERLAP = [256, 256, 512]
const IMDCT_TAIL = 16 // the entries of imdctOverlap[band] that carry into the next frame: its last 16
export const ENCODER_STATE_FLOATS = 483
export const DECODER_STATE_FLOATS = 179

function field(obj, name, what) {
  const v = obj === null || obj === undefined ? undefined : obj[name]
  if (v === null || v === undefined) throw new TypeError(`${what}: ${name} is missing`)
  return v
}
// copies a Float32Array-like of exactly `length` numbers into flat[at ..); TypeError naming the field otherwise
function take(flat, at, value, length, name) {
  const ok = value !== null && typeof value === 'object' && typeof value.length === 'number' &&
    (ArrayBuffer.isView(value) || Array.isArray(value))
  if (!ok) throw new TypeError(`${name} must be a Float32Array(${length})`)
  if (value.length !== length) throw new TypeError(`${name} must hold ${length} values, got ${value.length}`)
  for (let i = 0; i < length; i++) {
    if (typeof value[i] !== 'number') throw new TypeError(`${name}[${i}] is not a number`)
    flat[at + i] = value[i]
  }
  return at + length
}
function takeDelays(flat, obj, what) {
  const d = field(obj, 'qmfDelays', what)
  let at = take(flat, 0, field(d, 'lowBand', `${what}: qmfDelays`), QMF_DELAY, 'qmfDelays.lowBand')
  at = take(flat, at, field(d, 'midBand', `${what}: qmfDelays`), QMF_DELAY, 'qmfDelays.midBand')
  return take(flat, at, field(d, 'highBand', `${what}: qmfDelays`), QMF_HIGH_BAND_DELAY, 'qmfDelays.highBand')
}
function delaysOf(flat) {
  return { lowBand: flat.slice(0, 46), midBand: flat.slice(46, 92), highBand: flat.slice(92, 131) }
}

export class BufferPool {
  constructor() {
    this.encoderStream = null // c1_enc_stream, created by the first encode() closure call
    this.decoderStream = null // c1_dec_stream
    this.decoderPrecision = 'exact' // the precision of the decode() closure that created decoderStream (pipeline/decoder.js)
    this.encoderOptionsKey = null
    this.pendingEncoderState = null // Float32Array(483) set before the stream exists
    this.pendingDecoderState = null // Float32Array(179)
    this.qmfHistory = null // qmfAnalysisStage on its own: the previous frame's PCM (the QMF delay lines are made of it)
    this.transientBands = null // blockSelectorStage on its own: the bands of the last frame detection ran on (its magnitudes are transientDetection)
    this.mdctPreviousBands = null // mdctStage on its own: the previous frame's band samples (mdctOverlap is made of their tails)
    this.imdctPrevious = null // imdctStage on its own: the previous frame's coefficients and modes (imdctOverlap is made of them)
    this.synthesisPreviousBands = null // qmfSynthesisStage on its own: the previous frame's bands (qmfDelays are made of them)
  }

  // { qmfDelays: { lowBand, midBand, highBand }, mdctOverlap: [3 x Float32Array(32)], transientDetection: [Float32Array(64), (64), (128)] }
  getEncoderState() {
    const flat = this.encoderStream
      ? native().encStreamGetState(this.encoderStream, 1)
      : (this.pendingEncoderState ? this.pendingEncoderState.slice() : new Float32Array(ENCODER_STATE_FLOATS))
    const out = { qmfDelays: delaysOf(flat), mdctOverlap: [], transientDetection: [] }
    let at = 131
    for (const n of MDCT_OVERLAP) { out.mdctOverlap.push(flat.slice(at, at + n)); at += n }
    for (const n of TRANSIENT_BINS) { out.transientDetection.push(flat.slice(at, at + n)); at += n }
    return out
  }

  setEncoderState(state) {
    const what = 'setEncoderState'
    const flat = new Float32Array(ENCODER_STATE_FLOATS)
    let at = takeDelays(flat, state, what)
    const ov = field(state, 'mdctOverlap', what)
    const td = field(state, 'transientDetection', what)
    for (let b = 0; b < 3; b++) at = take(flat, at, ov[b], MDCT_OVERLAP[b], `mdctOverlap[${b}]`)
    for (let b = 0; b < 3; b++) at = take(flat, at, td[b], TRANSIENT_BINS[b], `transientDetection[${b}]`)
    if (this.encoderStream) native().encStreamSetState(this.encoderStream, 1, flat)
    else this.pendingEncoderState = flat
  }

  // { qmfDelays, imdctOverlap: [Float32Array(256), (256), (512)] }: the live 16 samples sit at the end of each array, where the
  // reference keeps them; the other entries are zeros on export and ignored on import
  getDecoderState() {
    const flat = this.decoderStream
      ? native().decStreamGetState(this.decoderStream, 1)
      : (this.pendingDecoderState ? this.pendingDecoderState.slice() : new Float32Array(DECODER_STATE_FLOATS))
    const out = { qmfDelays: delaysOf(flat), imdctOverlap: [] }
    for (let b = 0; b < 3; b++) {
      const a = new Float32Array(IMDCT_OVERLAP[b])
      a.set(flat.subarray(131 + IMDCT_TAIL * b, 131 + IMDCT_TAIL * (b + 1)), IMDCT_OVERLAP[b] - IMDCT_TAIL)
      out.imdctOverlap.push(a)
    }
    return out
  }

  setDecoderState(state) {
    const what = 'setDecoderState'
    const flat = new Float32Array(DECODER_STATE_FLOATS)
    let at = takeDelays(flat, state, what)
    const ov = field(state, 'imdctOverlap', what)
    for (let b = 0; b < 3; b++) {
      const whole = new Float32Array(IMDCT_OVERLAP[b])
      take(whole, 0, ov[b], IMDCT_OVERLAP[b], `imdctOverlap[${b}]`)
      flat.set(whole.subarray(IMDCT_OVERLAP[b] - IMDCT_TAIL), at)
      at += IMDCT_TAIL
    }
    if (this.decoderStream) native().decStreamSetState(this.decoderStream, 1, flat)
    else this.pendingDecoderState = flat
  }
}
