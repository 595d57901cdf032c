  float* X = CMP ? P1 : (kOwnX ? XX : AC);
  PSEC_DECL
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int S = r.S;
  const int tile = blockIdx.x;
  const int row0 = tile * RT;
  const int nrows = min(RT, r.B - row0);
  const float* P = r.params;
  constexpr int D = CMP ? kRingDC : ring_depth<TW>();  // CMP: 4 waves per SIMD hide more
  WRing<TW, D, 7, true, CMP> R;
  ring_setup(R, P, r.off, S, H, w * (H / NW), r.tiles);
  // the loss head's inputs and weights, loaded now so that their latency hides behind the
  // forward: lane l < RPW of wave w holds row RPW*w + l; the head weights of this wave's
  // output columns nb + 16t + (lane & 15).  The row indices of the head and of
  // the states gather go out first, then the rows they name, then the weight ring's prime
  // (vector memory completes in issue order: a gather behind the prime waited for it)
  const int hl = min(RPW * w + min(lane, RPW - 1), nrows - 1);
  float hz0, hz1, hold, hadv, hret, hq0, hq1;
  Gathered<RT, NT> xpre;
  const long hsrc = (long)r.idx[row0 + hl];
  gather_first<RT, NT, WIDE>(r.states, r.idx, S, nrows, row0, H, xpre);
  hz0 = r.pre_tanh[hsrc * 2];
  hz1 = r.pre_tanh[hsrc * 2 + 1];
  hold = r.old_logp[hsrc];
  hadv = r.adv[hsrc];
  hret = r.ret[hsrc];
  R.prime();
  const int nb = w * (H / NW);  // this wave's output columns of an H-wide layer
  f32x4 acc[RB][TW];
  // the squash correction depends on the stored pre-tanh actions only: computed here, its
  // latency hides behind the forward instead of lengthening the loss head's dependent chain
  hq0 = squash_corr(hz0);
  hq1 = squash_corr(hz1);
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
  // torch Normal: scale = exp(log_std); var = scale**2; log_scale = log(scale) -- parameters
  // only, so computed here, off the loss head's dependent chain (same bits)
  const float sc0 = expf(ls0), sc1 = expf(ls1);
  const float var0 = sc0 * sc0, var1 = sc1 * sc1;
  const float lsc0 = logf(sc0), lsc1 = logf(sc1);
  f32x4 av[RB][TW], cv[RB][TW];  // a1, c1 of this wave's columns (C layout)
  uint32_t mb[2] = {0u, 0u};      // CMP: ReLU decisions of h1, h2 (this lane's C elements)
  rows_forward<QH, NW, RT, true, D, 7, true, CMP, CMP, WIDE>(R, r.states, r.idx, S, nrows, row0, P,
                                                             r.off, X, H1, P1, AC, r.xg, r.h1,
                                                             r.h2, mb, av, cv PSEC_ARGS, &xpre);
  PSEC(3);
  const int g4 = lane >> 4, c16 = lane & 15;

  // ---- loss head (ppo/agent.py:226-245).  (1) each wave's partial dot products a1 . wa2 and
  // c1 . wc2 of every row over its columns, from the layer-3 accumulators (16-lane DPP sums);
  // (2) the per-row scalar part, RPW rows per wave (lane = row), the partials summed in wave
  // order; (3) dL/d[a1|c1] of this wave's columns into the [a1|c1] image for dh2 and ppo_wgrad,
  // and the head-parameter gradients of its columns summed over the rows
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
  PSEC(7);
  {
    const float LOG_SQRT_2PI = 0.91893853320467274178f;
    const float invB = 1.0f / (float)r.B;
    const float lo = 1.0f - r.eps_clip, hi = 1.0f + r.eps_clip;
    const int hr = RPW * w + min(lane, RPW - 1);  // this lane's row (lanes >= RPW: a copy)
    f32x4 dsum = HDOT[0][hr];
#pragma unroll
    for (int ww = 1; ww < NW; ++ww) dsum += HDOT[ww][hr];
    const float mu0 = dsum[0] + ba0, mu1 = dsum[1] + ba1, val = dsum[2] + bcv;
    const float d0 = hz0 - mu0, d1 = hz1 - mu1;
    const float lp0 = -(d0 * d0) / (2.0f * var0) - lsc0 - LOG_SQRT_2PI;
    const float lp1 = -(d1 * d1) / (2.0f * var1) - lsc1 - LOG_SQRT_2PI;
    const float logp = (lp0 - hq0) + (lp1 - hq1);
    const float log_ratio = logp - hold;
    const float ratio = expf(log_ratio);
    const float cr = fminf(fmaxf(ratio, lo), hi);
    const float s1 = ratio * hadv, s2 = cr * hadv;
    const float inr = (ratio >= lo && ratio <= hi) ? 1.0f : 0.0f;
    // torch.min / clamp backward: ties split the gradient evenly
    const float wsel = s1 < s2 ? 1.0f : (s1 > s2 ? inr : 0.5f * (1.0f + inr));
    const float dlogp = -invB * hadv * wsel * ratio;  // d(actor_loss)/d(logp)
    // rows past nrows (and lanes past RPW) contribute nothing
    const bool live = lane < RPW && hr < nrows;
    const float dmu0 = live ? dlogp * d0 / var0 : 0.0f;
    const float dmu1 = live ? dlogp * d1 / var1 : 0.0f;
    const float dv = live ? r.value_coef * 2.0f * (val - hret) * invB : 0.0f;
    if (lane < RPW) HROW[hr] = f32x4{dmu0, dmu1, dv, 0.0f};
    // this wave's rows' bias / log_std gradient terms and metrics, summed over its lanes in
    // lane order (the quad / half-row / row DPP tree over RPW <= 16 lanes)
    float tl[9] = {dmu0, dmu1, dv,
                   live ? dlogp * ((d0 * d0) / var0 - 1.0f) : 0.0f,
                   live ? dlogp * ((d1 * d1) / var1 - 1.0f) : 0.0f,
                   live ? -fminf(s1, s2) : 0.0f,
                   live ? (val - hret) * (val - hret) : 0.0f,
                   live ? (fabsf(ratio - 1.0f) > r.eps_clip ? 1.0f : 0.0f) : 0.0f,
                   live ? (ratio - 1.0f) - log_ratio : 0.0f};
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const float v = row16_sum(lane < 16 ? tl[k] : 0.0f);
      if (lane == 0) HTAIL[w][k] = v;
    }
    if (blockIdx.x == 0 && t == 0) {
      r.counters[0] += 1;  // Adam step t for this minibatch
      r.counters[1] += 1;  // metrics row (this step writes row counters[1]-1)
    }
  }
  __syncthreads();
  PSEC(11);
  {
    // dac of this wave's columns (the reference's expression per element), and the head
    // weight gradients sum_rows dmu * a1 / dv * c1 of its columns: per lane over its rows, then
    // over the four 16-lane groups
    float ga0[TW], ga1[TW], gc[TW];
#pragma unroll
    for (int u = 0; u < TW; ++u) ga0[u] = ga1[u] = gc[u] = 0.0f;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = 16 * rb + 4 * g4 + q;
        const f32x4 sc = HROW[row];
        const float dmu0 = sc[0], dmu1 = sc[1], dv = sc[2];
        float* arow = AC + row * PA;
#pragma unroll
        for (int u = 0; u < TW; ++u) {
          const int col = nb + 16 * u + c16;
          const float a = av[rb][u][q], cc = cv[rb][u][q];
          arow[col] = a > 0.0f ? (dmu0 * wa0[u] + dmu1 * wa1[u]) : 0.0f;
          arow[H + col] = cc > 0.0f ? dv * wc[u] : 0.0f;
          ga0[u] += dmu0 * a;
          ga1[u] += dmu1 * a;
          gc[u] += dv * cc;
        }
      }
    float* out = r.head_part + (long)tile * r.HP;
#pragma unroll
    for (int u = 0; u < TW; ++u) {
      // lanes c, c+16, c+32, c+48 hold the same column: (g0 + g1) + (g2 + g3)
      ga0[u] += __shfl_xor(ga0[u], 16);
      ga1[u] += __shfl_xor(ga1[u], 16);
      gc[u] += __shfl_xor(gc[u], 16);
      ga0[u] += __shfl_xor(ga0[u], 32);
      ga1[u] += __shfl_xor(ga1[u], 32);
      gc[u] += __shfl_xor(gc[u], 32);
      if (g4 == 0) {
        const int col = nb + 16 * u + c16;
        out[col] = ga0[u];
        out[H + col] = ga1[u];
        out[2 * H + col] = gc[u];
      }
    }
    if (w == 0 && lane < 9) {  // the waves' tail sums in wave order
      float v = HTAIL[0][lane];
#pragma unroll
      for (int ww = 1; ww < NW; ++ww) v += HTAIL[ww][lane];
      out[3 * H + lane] = v;
    }
  }
  __syncthreads();
  rows_out<NT, RT>(AC, PA, r.dac + (long)row0 * 2 * H, 2 * H, 2 * H, nrows);
  PSEC(4);
  // dh2 = (dac [Wa1; Wc1]) * (h2 > 0)   ([Wa1; Wc1] is [2H][H]: k-major); the two halves of
  // K = 2H (Wa1 rows, Wc1 rows) are summed at the end
  zero_acc(acc);
  R.template run<4>(AC, PA, acc);
  R.template run<5>(AC + H, PA, acc);
  float* const DH2 = CMP ? H1 : H2;  // CMP: P0
  float* const DH1 = CMP ? P1 : H1;
  if constexpr (CMP) {
    __syncthreads();  // every wave has read dac (P0 | P1)
    row_epi_maskbits(acc, mb[1], DH2, PH, nb);
  } else {
    row_epi_mask(acc, H2, PH, nb);
  }
  __syncthreads();
  if (r.dh2) rows_out<NT, RT>(DH2, PH, r.dh2 + (long)row0 * H, H, H, nrows);
  PSEC(5);
  // dh1 = (dh2 W2) * (h1 > 0)
  zero_acc(acc);
  R.template run<6>(DH2, PH, acc);
  if constexpr (CMP)
    row_epi_maskbits(acc, mb[0], DH1, PH, nb);  // P1: dac is dead, dh2 is in P0
  else
    row_epi_mask(acc, H1, PH, nb);  // dh1 over h1 (same thread)
  __syncthreads();
  if (r.dh1) rows_out<NT, RT>(DH1, PH, r.dh1 + (long)row0 * H, H, H, nrows);
  PSEC(6);
  PSEC_FLUSH;
