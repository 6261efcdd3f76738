// c1_qmf_frame.inc -- qmfAnalysisStage (encoder.js:57-96) of one frame, for the body of a frame loop in which one wave walks
// consecutive frames of one channel and carries the delay lines in LDS.  Included textually by k_detect_features
// (c1_k_detect.hip) and k_qmf_bands (c1_k_modes.hip): the two kernels run the same statements in the same order, and the
// compiler sees them exactly where a hand-written body would stand (as a function taking the LDS image by reference the
// same code came out of the compiler with other registers and operand orders in k_detect_features, whose ISA is pinned).
//
// Names the including loop provides:
//   S               the wave's LDS image: double d1[46], d2[46] (delay lines of the two stages), float hbuf[296] (the high band
//                   behind its 39-sample delay, [0, 39) = tail of the previous frame), float band[512] (low | mid | high),
//                   double u.q1.w1[698] and u.q2.w2[454] (work buffers, pidx<3> / pidx<2>; they may share storage)
//   lane, T         lane_for_this_frame / tables_for_this_frame of this frame
//   pre_a, pre_b    v4f: PCM samples 4 lane .. and 256 + 4 lane .. of frame f, delivered; on exit frame f + 1's, REQUESTED only
//   pcm, f, f_end   the channel's PCM, this frame, the end of the run
// On exit S.band holds the frame's bands, the delay lines stand at the next frame, the wave runs at priority 1, and the last
// LDS write (hbuf[0, 39)) is not fenced yet.  The includer takes delivery of pre_a / pre_b (asm volatile("" : "+v"(..))) at a
// point every path to the top of its loop passes, before it issues the frame's stores: loads and stores share one in-order
// counter on this part.
    {
      const v4f a = pre_a, b = pre_b;
      double *w1 = S.u.q1.w1;
      if (lane < 46) w1[pidx<3>(lane)] = S.d1[lane];
      const int e0 = 46 + 4 * lane;
      *reinterpret_cast<double2 *>(&w1[pidx<3>(e0)]) = make_double2((double)a.x, (double)a.y);
      *reinterpret_cast<double2 *>(&w1[pidx<3>(e0 + 2)]) = make_double2((double)a.z, (double)a.w);
      *reinterpret_cast<double2 *>(&w1[pidx<3>(e0 + 256)]) = make_double2((double)b.x, (double)b.y);
      *reinterpret_cast<double2 *>(&w1[pidx<3>(e0 + 258)]) = make_double2((double)b.z, (double)b.w);
    }
    wave_fence();
    {
      // the next frame's PCM (the last frame asks for itself again: under a condition the loaded values are copied into the
      // loop-carried registers behind the load, i.e. waited for on the spot)
      const v4f *p4 = reinterpret_cast<const v4f *>(pcm + ((f + 1 < f_end) ? f + 1 : f) * 512);
      pre_a = p4[lane]; pre_b = p4[64 + lane];
    }
    {
      double ev[4], od[4];
      __builtin_amdgcn_s_setprio(3);   // wave priorities as in k_analysis_fast: QMF cores 3, transient FFT 0, the rest 1
      if (own_block()) qmf_analysis_core<4, 3>(S.u.q1.w1, lane, T, ev, od); else { for (int d = 0; d < 4; d++) { ev[d] = S.u.q1.w1[lane + d]; od[d] = 1.0; } }
      double *w2 = S.u.q2.w2;
      if (lane < 46) { w2[pidx<2>(lane)] = S.d2[lane]; S.d1[lane] = S.u.q1.w1[pidx<3>(512 + lane)]; }
      float lo[4];
#pragma unroll
      for (int d = 0; d < 4; d++) {
        lo[d] = f32(ev[d] + od[d]);
        S.hbuf[39 + 4 * lane + d] = f32(ev[d] - od[d]);
      }
      *reinterpret_cast<double2 *>(&w2[pidx<2>(46 + 4 * lane)]) = make_double2((double)lo[0], (double)lo[1]);
      *reinterpret_cast<double2 *>(&w2[pidx<2>(48 + 4 * lane)]) = make_double2((double)lo[2], (double)lo[3]);
    }
    wave_fence();
    {
      double ev[2], od[2];
      if (own_block()) qmf_analysis_core<2, 2>(S.u.q2.w2, lane, T, ev, od); else { for (int d = 0; d < 2; d++) { ev[d] = S.u.q2.w2[lane + d]; od[d] = 1.0; } }
      __builtin_amdgcn_s_setprio(1);
      *reinterpret_cast<float2 *>(&S.band[2 * lane]) = make_float2(f32(ev[0] + od[0]), f32(ev[1] + od[1]));
      *reinterpret_cast<float2 *>(&S.band[128 + 2 * lane]) = make_float2(f32(ev[0] - od[0]), f32(ev[1] - od[1]));
      *reinterpret_cast<float4 *>(&S.band[256 + 4 * lane]) = *reinterpret_cast<const float4 *>(&S.hbuf[4 * lane]);
      if (lane < 46) S.d2[lane] = S.u.q2.w2[pidx<2>(256 + lane)];
    }
    wave_fence();
    {
      float keep = 0.0f;
      if (lane < 39) keep = S.hbuf[256 + lane];
      wave_fence();
      if (lane < 39) S.hbuf[lane] = keep;
    }
