  float* const H1 = P01;            // P0
  float* const P1 = P01 + RT * PH;  // the states, then h2
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int row0 = blockIdx.x * RT;
  const int nrows = min(RT, r.B - row0);
#ifdef HWY_PPO_VMASK_TU
  // hwy_ppo_value_masked: a tile without a marked row stores zeros before any weight is read
  const uint64_t vmask = vmask_tile(r, row0, nrows, lane);
  if (!vmask) {
    if (t < nrows) r.value[row0 + t] = 0.0f;
    return;
  }
#endif
  const float* P = r.params;
  constexpr int D = kRingDC;
  WRing<TW, D, 4, true, true> R;
  ring_setup(R, P, r.off, r.S, H, w * (H / NW), r.tiles);
  Gathered<RT, 64 * NW> xpre;  // the states rows, issued before the ring's prime (rows_body)
  gather_first<RT, 64 * NW, WIDE>(r.states, nullptr, r.S, nrows, row0, H, xpre);
  R.prime();
#ifdef HWY_SECTION_PROFILE
  uint64_t _pt = 0, _pacc[16];
#endif
  float wa0[TW], wa1[TW], wc[TW];
#pragma unroll
  for (int u = 0; u < TW; ++u) {
    const int col = w * (H / NW) + 16 * u + (lane & 15);
    wa0[u] = P[r.off[P_WA2] + col];
    wa1[u] = P[r.off[P_WA2] + H + col];
    wc[u] = P[r.off[P_WC2] + col];
  }
  const float ba0 = P[r.off[P_BA2]], ba1 = P[r.off[P_BA2] + 1], bcv = P[r.off[P_BC2]];
  const float ls0 = P[r.off[P_LOGSTD]], ls1 = P[r.off[P_LOGSTD] + 1];
  // this lane's head row (lanes < RPW of wave w: row RPW w + lane) and its noise
  const int hr = RPW * w + min(lane, RPW - 1);
  const bool live = lane < RPW && hr < nrows;
  const long b = row0 + min(hr, nrows - 1);
  float n0 = 0.0f, n1 = 0.0f;
  if (r.noise) n0 = r.noise[2 * b], n1 = r.noise[2 * b + 1];
  f32x4 av[RB][TW], cv[RB][TW];
  uint32_t mb[2] = {0u, 0u};
  rows_forward<QH, NW, RT, true, D, 4, true, false, true, WIDE>(
      R, r.states, nullptr, r.S, nrows, row0, P, r.off, P1, H1, P1, nullptr, nullptr, nullptr,
      nullptr, mb, av, cv PSEC_ARGS, &xpre);
  const int g4 = lane >> 4, c16 = lane & 15;
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float p0 = 0.0f, p1 = 0.0f, pv = 0.0f;
#pragma unroll
      for (int u = 0; u < TW; ++u) {
        p0 += av[rb][u][q] * wa0[u];
        p1 += av[rb][u][q] * wa1[u];
        pv += cv[rb][u][q] * wc[u];
      }
      p0 = row16_sum(p0), p1 = row16_sum(p1), pv = row16_sum(pv);
      if (c16 == 0) HDOT[w][16 * rb + 4 * g4 + q] = f32x4{p0, p1, pv, 0.0f};
    }
  __syncthreads();
  if (!live) return;
  f32x4 dsum = HDOT[0][hr];
#pragma unroll
  for (int ww = 1; ww < NW; ++ww) dsum += HDOT[ww][hr];
#ifdef HWY_PPO_VMASK_TU
  r.value[b] = ((vmask >> hr) & 1ull) ? dsum[2] + bcv : 0.0f;
  (void)ba0, (void)ba1, (void)ls0, (void)ls1, (void)n0, (void)n1;
#else
  const float mu0 = dsum[0] + ba0, mu1 = dsum[1] + ba1, val = dsum[2] + bcv;
  float z0 = mu0, z1 = mu1, lp = 0.0f;
  if (r.noise) {
    // torch Normal: scale = exp(log_std); var = scale**2; log_scale = log(scale)
    const float sc0 = expf(ls0), sc1 = expf(ls1);
    const float var0 = sc0 * sc0, var1 = sc1 * sc1;
    const float lsc0 = logf(sc0), lsc1 = logf(sc1);
    const float LOG_SQRT_2PI = 0.91893853320467274178f;
    z0 = mu0 + sc0 * n0;
    z1 = mu1 + sc1 * n1;
    const float d0 = z0 - mu0, d1 = z1 - mu1;
    const float t0 = tanhf(z0), t1 = tanhf(z1);
    const float lp0 = -(d0 * d0) / (2.0f * var0) - lsc0 - LOG_SQRT_2PI;
    const float lp1 = -(d1 * d1) / (2.0f * var1) - lsc1 - LOG_SQRT_2PI;
    lp = (lp0 - log1pf(-(t0 * t0) + 1e-6f)) + (lp1 - log1pf(-(t1 * t1) + 1e-6f));
  }
  r.action[2 * b] = tanhf(z0);
  r.action[2 * b + 1] = tanhf(z1);
  r.pre_tanh[2 * b] = z0;
  r.pre_tanh[2 * b + 1] = z1;
  r.logp[b] = lp;
  r.value[b] = val;
#endif
