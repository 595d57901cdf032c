  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int row0 = blockIdx.x * kRowTile;
  const int nrows = min(kRowTile, r.B - row0);
#ifdef HWY_PPO_VMASK_TU
  // hwy_ppo_value_masked: a tile without a marked row stores zeros before any weight is read
  const uint64_t vmask = vmask_tile(r, row0, nrows, lane);
  if (!vmask) {
    if (t < nrows) r.value[row0 + t] = 0.0f;
    return;
  }
#endif
  const float* P = r.params;
  constexpr int TW = H_TW(QH, NW);
  constexpr int D = ring_depth<TW>();
  WRing<TW, D, 4, TL> R;
  ring_setup(R, P, r.off, r.S, H, w * (H / NW), r.tiles);
  R.prime();
#ifdef HWY_SECTION_PROFILE
  uint64_t _pt = 0, _pacc[16];
#endif
  f32x4 unused_a[kRowTile / 16][TW], unused_c[kRowTile / 16][TW];
  uint32_t unused_m[2];
  rows_forward<QH, NW, kRowTile, false, D, 4, TL, false, false, WIDE>(
      R, r.states, nullptr, r.S, nrows, row0, P, r.off, X, H1, H2, AC, nullptr, nullptr, nullptr,
      unused_m, unused_a, unused_c PSEC_ARGS);
  float wa0[QH], wa1[QH], wc[QH];
#pragma unroll
  for (int q = 0; q < QH; ++q) {
    const int col = lane + 64 * q;
    wa0[q] = P[r.off[P_WA2] + col];
    wa1[q] = P[r.off[P_WA2] + H + col];
    wc[q] = P[r.off[P_WC2] + col];
  }
  const float ba0 = P[r.off[P_BA2]], ba1 = P[r.off[P_BA2] + 1], bcv = P[r.off[P_BC2]];
  const float ls0 = P[r.off[P_LOGSTD]], ls1 = P[r.off[P_LOGSTD] + 1];
  const float sc0 = expf(ls0), sc1 = expf(ls1);
  const float var0 = sc0 * sc0, var1 = sc1 * sc1;
  const float lsc0 = logf(sc0), lsc1 = logf(sc1);
  const float LOG_SQRT_2PI = 0.91893853320467274178f;
  for (int rr = 0; rr < RPW; ++rr) {
    const int lr = RPW * w + rr;
    if (lr >= nrows) break;
    const int b = row0 + lr;
    const float* arow = AC + lr * PA;
    float p0 = 0.0f, p1 = 0.0f, pv = 0.0f;
#pragma unroll
    for (int q = 0; q < QH; ++q) {
      const int col = lane + 64 * q;
      const float a = arow[col], c = arow[H + col];
      p0 += a * wa0[q];
      p1 += a * wa1[q];
      pv += c * wc[q];
    }
    const float mu0 = wave_sum_dpp(p0) + ba0, mu1 = wave_sum_dpp(p1) + ba1,
                val = wave_sum_dpp(pv) + bcv;
#ifdef HWY_PPO_VMASK_TU
    if (lane == 0) r.value[b] = ((vmask >> lr) & 1ull) ? val : 0.0f;
    (void)mu0, (void)mu1, (void)var0, (void)var1, (void)lsc0, (void)lsc1, (void)LOG_SQRT_2PI;
#else
    if (lane == 0) {
      float z0 = mu0, z1 = mu1, lp = 0.0f;
      if (r.noise) {
        z0 = mu0 + sc0 * r.noise[2 * (long)b];
        z1 = mu1 + sc1 * r.noise[2 * (long)b + 1];
        const float d0 = z0 - mu0, d1 = z1 - mu1;
        const float t0 = tanhf(z0), t1 = tanhf(z1);
        const float lp0 = -(d0 * d0) / (2.0f * var0) - lsc0 - LOG_SQRT_2PI;
        const float lp1 = -(d1 * d1) / (2.0f * var1) - lsc1 - LOG_SQRT_2PI;
        lp = (lp0 - log1pf(-(t0 * t0) + 1e-6f)) + (lp1 - log1pf(-(t1 * t1) + 1e-6f));
      }
      r.action[2 * (long)b] = tanhf(z0);
      r.action[2 * (long)b + 1] = tanhf(z1);
      r.pre_tanh[2 * (long)b] = z0;
      r.pre_tanh[2 * (long)b + 1] = z1;
      r.logp[b] = lp;
      r.value[b] = val;
    }
#endif
  }
