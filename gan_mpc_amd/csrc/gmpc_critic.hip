// Critic (discriminator) LSTM sweeps for the shapes gmpc_critic_lstm.hip does not cover: LSTM(F) over the T+1 rows
// of each sequence forward, BPTT backward.
//   F = 64: k_lstm_fwd / k_lstm_bwd ("first generation"), any input width n with n + F <= 256 beyond the second
//           generation's n <= 32, and the recurrent half of the wide-input path (cd.n == 0, Wcat = Wh, x_t Wx formed
//           by a GEMM beforehand and handed over as xproj);
//   any other F <= 128: the strided k_lstm_fwd_g / k_lstm_bwd_g.
// The head (k_head2) is in gmpc_critic_lstm.hip, the weight-gradient GEMMs in gmpc_wgrad.hip, clip + Adam in
// gmpc_optim.hip.
//
// Reference arithmetic: critic/nn.py:28-42 (flax OptimizedLSTMCell scanned over the sequence, zero
// carry, gate order i,f,g,o), gan/js_policy.py:41-68 (losses).
//
// Layout of the F = 64 kernels: a workgroup of 256 threads owns 4 sequences for the whole sweep.  Thread j
// produces gate pre-activation j (4F = 256) for the 4 sequences from the concatenated kernel Wcat = [Wx; Wh]
// ((n+F) x 4F, exactly the flat critic layout), streamed from L2 every step; the cell update runs as thread
// (unit, sequence).  Saved per (sequence, step): activated gates, c_t, h_{t-1}.
// (Measured on MI355X: keeping [Wx; Wh] in LDS for the whole sweep does not pay, 0.25 -> 0.28 ms: the step is bound
// by instruction issue -- transcendentals + FMAs at one wave per SIMD -- not by the L2 weight stream.)
#include "gmpc_launch.h"

__global__ __launch_bounds__(GMPC_THREADS) void k_lstm_fwd(int Bc, CriticDesc cd, const float* xseq,
                                                           float* gates, float* cs, float* hp,
                                                           float* hT, const float* xproj) {
  constexpr int SB = 4;                                     // sequences per workgroup
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* act = reinterpret_cast<float4*>(smem);            // [n + F]: x_t, then h_{t-1}
  float4* gbuf = act + (cd.n + cd.F);                       // [4F] activated gates
  const int tid = threadIdx.x;
  const int n = cd.n, F = cd.F, T1 = cd.T1, G4 = 4 * F, K = n + F;
  const int s0 = blockIdx.x * SB;
  const int u = tid % F, grp = tid / F;       // cell-update role: unit u of sequence grp (F*4 == blockDim)
  float c = 0.f;
  float* actf = reinterpret_cast<float*>(act);
  float* gbf = reinterpret_cast<float*>(gbuf);
  for (int e = tid; e < F * SB; e += blockDim.x) actf[n * SB + e] = 0.f;   // h_{-1} = 0
  const float bj = tid < G4 ? cd.b[tid] : 0.f;
  // x_t of the next step is requested one step ahead when one element per thread covers it
  const bool xpf = n * SB <= (int)blockDim.x;
  const int xsb = tid / (n > 0 ? n : 1), xi = tid - xsb * n;
  const bool xon = xpf && tid < n * SB;
  const float* xptr = xseq + ((size_t)min(s0 + (xon ? xsb : 0), Bc - 1) * T1) * n + (xon ? xi : 0);
  float xnext = xon ? xptr[0] : 0.f;
  for (int t = 0; t < T1; ++t) {
    if (xpf) {
      if (xon) {
        actf[xi * SB + xsb] = xnext;
        if (t + 1 < T1) xnext = xptr[(size_t)(t + 1) * n];
      }
    } else {
      for (int e = tid; e < n * SB; e += blockDim.x) {
        const int sb = e / n, i = e - sb * n;
        const int s = min(s0 + sb, Bc - 1);
        actf[i * SB + sb] = xseq[((size_t)s * T1 + t) * n + i];
      }
    }
    __syncthreads();
    // save h_{t-1}
    for (int e = tid; e < F * SB; e += blockDim.x) {
      const int sb = e / F, k = e - sb * F;
      if (s0 + sb < Bc) hp[((size_t)(s0 + sb) * T1 + t) * F + k] = actf[(n + k) * SB + sb];
    }
    float4 acc[1] = {make_float4(bj, bj, bj, bj)};
    if (xproj != nullptr && tid < G4) {
      // wide inputs: x_t Wx was formed by a GEMM beforehand (cd.n == 0 here, Wcat = Wh)
      float v[4];
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        const int sq = min(s0 + cc, Bc - 1);
        v[cc] = xproj[((size_t)sq * T1 + t) * G4 + tid];
      }
      acc[0] = make_float4(bj + v[0], bj + v[1], bj + v[2], bj + v[3]);
    }
    dense_rows<1>(cd.Wcat, K, G4, tid, act, acc);
    if (tid < G4) {
      const bool is_g = (tid >= 2 * F) && (tid < 3 * F);
      float4 v = acc[0];
      if (is_g) { v.x = tanhf(v.x); v.y = tanhf(v.y); v.z = tanhf(v.z); v.w = tanhf(v.w); }
      else { v.x = sigmoidf_(v.x); v.y = sigmoidf_(v.y); v.z = sigmoidf_(v.z); v.w = sigmoidf_(v.w); }
      gbuf[tid] = v;
#pragma unroll
      for (int cc = 0; cc < 4; ++cc)
        if (s0 + cc < Bc) gates[((size_t)(s0 + cc) * T1 + t) * G4 + tid] = f4get(v, cc);
    }
    __syncthreads();
    const float ig = gbf[(0 * F + u) * SB + grp], fg = gbf[(1 * F + u) * SB + grp];
    const float gg = gbf[(2 * F + u) * SB + grp], og = gbf[(3 * F + u) * SB + grp];
    c = fg * c + ig * gg;
    const float h = og * tanhf(c);
    actf[(n + u) * SB + grp] = h;
    if (s0 + grp < Bc) {
      cs[((size_t)(s0 + grp) * T1 + t) * F + u] = c;
      if (t == T1 - 1) hT[(size_t)(s0 + grp) * F + u] = h;
    }
    __syncthreads();
  }
}

// (The head -- forward, loss, backward -- is k_head2 in gmpc_critic_lstm.hip for every shape.)

__global__ __launch_bounds__(GMPC_THREADS) void k_lstm_bwd(int Bc, CriticDesc cd, const float* gates,
                                                           const float* cs, const float* dhT,
                                                           float* dz, float* dxseq) {
  constexpr int SB = 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* dzb = reinterpret_cast<float4*>(smem);            // [4F] of the GMPC_THREADS + 128 float4 of each half
  float4* part = dzb + (GMPC_THREADS + 128);                // dense_small scratch / result
  const int tid = threadIdx.x;
  const int n = cd.n, F = cd.F, T1 = cd.T1, G4 = 4 * F, K = n + F;
  const int s0 = blockIdx.x * SB;
  const int u = tid % F, sb = tid / F;        // unit u of sequence sb
  const int s = min(s0 + sb, Bc - 1);
  float* dzf = reinterpret_cast<float*>(dzb);
  float dh = dhT[(size_t)s * F + u], dc = 0.f;
  // the saved gates and cell states of step t - 1 are requested while step t is processed: the sweep
  // never waits for a global round trip (the cell state of t - 1 is also step t's c_prev)
  float pg[4], pc;
  auto pf_load = [&](int t) {
    const size_t gb = ((size_t)s * T1 + t) * G4;
    pg[0] = gates[gb + u]; pg[1] = gates[gb + F + u];
    pg[2] = gates[gb + 2 * F + u]; pg[3] = gates[gb + 3 * F + u];
    pc = t > 0 ? cs[((size_t)s * T1 + t - 1) * F + u] : 0.f;
  };
  float ccur = cs[((size_t)s * T1 + T1 - 1) * F + u];
  pf_load(T1 - 1);
  for (int t = T1 - 1; t >= 0; --t) {
    const float ig = pg[0], fg = pg[1], gg = pg[2], og = pg[3];
    const float cprev = pc;
    if (t > 0) pf_load(t - 1);
    const float ct = ccur;
    ccur = cprev;
    const float tc = tanhf(ct);
    const float d_o = dh * tc;
    dc = dc + dh * og * (1.f - tc * tc);
    const float di = dc * gg, df_ = dc * cprev, dg = dc * ig;
    const float zi = di * ig * (1.f - ig), zf = df_ * fg * (1.f - fg), zg = dg * (1.f - gg * gg),
                zo = d_o * og * (1.f - og);
    dzf[(0 * F + u) * SB + sb] = zi;
    dzf[(1 * F + u) * SB + sb] = zf;
    dzf[(2 * F + u) * SB + sb] = zg;
    dzf[(3 * F + u) * SB + sb] = zo;
    if (s0 + sb < Bc && dz != nullptr) {
      float* d = dz + ((size_t)s * T1 + t) * G4;
      d[u] = zi; d[F + u] = zf; d[2 * F + u] = zg; d[3 * F + u] = zo;
    }
    dc = dc * fg;
    __syncthreads();
    // [dx ; dh_prev][k][sb] = sum_j WcatT[j][k] dz[j][sb]
    dense_small<1>(cd.WcatT, G4, K, dzb, part);
    const float* pf = reinterpret_cast<const float*>(part);
    dh = pf[(n + u) * SB + sb];
    if (dxseq != nullptr) {
      for (int e = tid; e < n * SB; e += blockDim.x) {
        const int sq = e / n, i = e - sq * n;
        if (s0 + sq < Bc) dxseq[((size_t)(s0 + sq) * T1 + t) * n + i] = pf[i * SB + sq];
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// Any lstm_features F <= 128 (the reference makes it a yaml integer, critic/nn.py:11, config/gan_hyperparameters.yaml:
// 60-65; its expert model uses 128): the kernels above and gmpc_critic_lstm.hip are built around 4 F = 256 = one
// workgroup.  Here the 4 F gate columns and the F cell units are strided over the 256 threads; weights come from L2
// (coalesced over the gate column / the input row), expf / tanhf activations.  4 sequences per workgroup, one float4
// per (row, 4 sequences) in LDS.  Same saves as k_lstm_fwd (activated gates, c_t, h_{t-1}) so that the weight-gradient
// GEMMs, the head and the wide-input path (cd.n == 0, Wcat = Wh, x Wx from xproj) are shared.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GMPC_THREADS) void k_lstm_fwd_g(int Bc, CriticDesc cd, const float* xseq, float* gates,
                                                             float* cs, float* hp, float* hT, const float* xproj) {
  extern __shared__ __attribute__((aligned(16))) char smem_g[];
  const int tid = threadIdx.x;
  const int n = cd.n, F = cd.F, T1 = cd.T1, G4 = 4 * F, K = n + F;
  float4* act = reinterpret_cast<float4*>(smem_g);          // [n + F]: x_t, then h_{t-1}
  float4* gbuf = act + K;                                   // [4 F] activated gates
  float4* cst = gbuf + G4;                                  // [F] cell state
  float* actf = reinterpret_cast<float*>(act);
  const int s0 = blockIdx.x * 4;
  int sq[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) sq[c] = min(s0 + c, Bc - 1);
  for (int e = tid; e < F; e += GMPC_THREADS) {
    act[n + e] = make_float4(0.f, 0.f, 0.f, 0.f);
    cst[e] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (int t = 0; t < T1; ++t) {
    for (int e = tid; e < n * 4; e += GMPC_THREADS) {
      const int i = e >> 2, c = e & 3;
      actf[e] = xseq[((size_t)sq[c] * T1 + t) * n + i];
    }
    __syncthreads();
    for (int e = tid; e < F * 4; e += GMPC_THREADS) {       // save h_{t-1}
      const int k = e >> 2, c = e & 3;
      if (s0 + c < Bc) hp[((size_t)(s0 + c) * T1 + t) * F + k] = actf[(n + k) * 4 + c];
    }
    for (int j = tid; j < G4; j += GMPC_THREADS) {
      const float bj = cd.b[j];
      float4 acc[1] = {make_float4(bj, bj, bj, bj)};
      if (xproj != nullptr) {
        acc[0].x += xproj[((size_t)sq[0] * T1 + t) * G4 + j];
        acc[0].y += xproj[((size_t)sq[1] * T1 + t) * G4 + j];
        acc[0].z += xproj[((size_t)sq[2] * T1 + t) * G4 + j];
        acc[0].w += xproj[((size_t)sq[3] * T1 + t) * G4 + j];
      }
      dense_rows<1>(cd.Wcat, K, G4, j, act, acc);
      float4 v = acc[0];
      if (j / F == 2) { v.x = tanhf(v.x); v.y = tanhf(v.y); v.z = tanhf(v.z); v.w = tanhf(v.w); }
      else { v.x = sigmoidf_(v.x); v.y = sigmoidf_(v.y); v.z = sigmoidf_(v.z); v.w = sigmoidf_(v.w); }
      gbuf[j] = v;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (s0 + c < Bc) gates[((size_t)(s0 + c) * T1 + t) * G4 + j] = f4get(v, c);
    }
    __syncthreads();
    for (int u = tid; u < F; u += GMPC_THREADS) {
      const float4 ig = gbuf[u], fg = gbuf[F + u], gg = gbuf[2 * F + u], og = gbuf[3 * F + u];
      float4 c = cst[u], h;
      c.x = fg.x * c.x + ig.x * gg.x; c.y = fg.y * c.y + ig.y * gg.y;
      c.z = fg.z * c.z + ig.z * gg.z; c.w = fg.w * c.w + ig.w * gg.w;
      h.x = og.x * tanhf(c.x); h.y = og.y * tanhf(c.y); h.z = og.z * tanhf(c.z); h.w = og.w * tanhf(c.w);
      cst[u] = c;
      act[n + u] = h;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (s0 + q < Bc) {
          cs[((size_t)(s0 + q) * T1 + t) * F + u] = f4get(c, q);
          if (t == T1 - 1) hT[(size_t)(s0 + q) * F + u] = f4get(h, q);
        }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(GMPC_THREADS) void k_lstm_bwd_g(int Bc, CriticDesc cd, const float* gates, const float* cs,
                                                             const float* dhT, float* dz, float* dxseq) {
  extern __shared__ __attribute__((aligned(16))) char smem_g[];
  const int tid = threadIdx.x;
  const int n = cd.n, F = cd.F, T1 = cd.T1, G4 = 4 * F, K = n + F;
  float4* dzb = reinterpret_cast<float4*>(smem_g);          // [4 F]
  float4* dhb = dzb + G4;                                   // [F] dh_t
  float4* dcb = dhb + F;                                    // [F] dc
  const int s0 = blockIdx.x * 4;
  int sq[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) sq[c] = min(s0 + c, Bc - 1);
  for (int u = tid; u < F; u += GMPC_THREADS) {
    dhb[u] = make_float4(dhT[(size_t)sq[0] * F + u], dhT[(size_t)sq[1] * F + u], dhT[(size_t)sq[2] * F + u],
                         dhT[(size_t)sq[3] * F + u]);
    dcb[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  for (int t = T1 - 1; t >= 0; --t) {
    for (int u = tid; u < F; u += GMPC_THREADS) {
      float zi[4], zf[4], zg[4], zo[4], dcn[4];
      const float4 dh4 = dhb[u], dc4 = dcb[u];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const size_t gb = ((size_t)sq[c] * T1 + t) * G4;
        const float ig = gates[gb + u], fg = gates[gb + F + u], gg = gates[gb + 2 * F + u], og = gates[gb + 3 * F + u];
        const float ct = cs[((size_t)sq[c] * T1 + t) * F + u];
        const float cprev = t > 0 ? cs[((size_t)sq[c] * T1 + t - 1) * F + u] : 0.f;
        const float tc = tanhf(ct);
        const float dh = f4get(dh4, c);
        const float d_o = dh * tc;
        const float dc = f4get(dc4, c) + dh * og * (1.f - tc * tc);
        const float di = dc * gg, df_ = dc * cprev, dg = dc * ig;
        zi[c] = di * ig * (1.f - ig); zf[c] = df_ * fg * (1.f - fg); zg[c] = dg * (1.f - gg * gg);
        zo[c] = d_o * og * (1.f - og);
        dcn[c] = dc * fg;
        if (s0 + c < Bc && dz != nullptr) {
          float* d = dz + gb;
          d[u] = zi[c]; d[F + u] = zf[c]; d[2 * F + u] = zg[c]; d[3 * F + u] = zo[c];
        }
      }
      dzb[u] = make_float4(zi[0], zi[1], zi[2], zi[3]);
      dzb[F + u] = make_float4(zf[0], zf[1], zf[2], zf[3]);
      dzb[2 * F + u] = make_float4(zg[0], zg[1], zg[2], zg[3]);
      dzb[3 * F + u] = make_float4(zo[0], zo[1], zo[2], zo[3]);
      dcb[u] = make_float4(dcn[0], dcn[1], dcn[2], dcn[3]);
    }
    __syncthreads();
    // [dx ; dh_{t-1}][k] = sum_j WcatT[j][k] dz[j]   (WcatT: [4 F][n + F], coalesced over k)
    for (int k = tid; k < K; k += GMPC_THREADS) {
      float4 acc[1] = {make_float4(0.f, 0.f, 0.f, 0.f)};
      dense_rows<1>(cd.WcatT, G4, K, k, dzb, acc);
      if (k < n) {
        if (dxseq != nullptr) {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (s0 + c < Bc) dxseq[((size_t)(s0 + c) * T1 + t) * n + k] = f4get(acc[0], c);
        }
      } else {
        dhb[k - n] = acc[0];
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// host-side launchers: one workgroup per 4 sequences
// ---------------------------------------------------------------------------------------------
void gmpc_launch_lstm_fwd(int Bc, const CriticDesc& cd, const float* xseq, float* gates, float* cs,
                          float* hp, float* hT, const float* xproj, hipStream_t s) {
  const int grid = (Bc + 3) / 4;
  if (cd.F != 64) {       // the strided form for other feature counts
    hipLaunchKernelGGL(k_lstm_fwd_g, dim3(grid), dim3(GMPC_THREADS),
                       ((size_t)cd.n + 6 * (size_t)cd.F) * sizeof(float4), s, Bc, cd, xseq, gates, cs, hp, hT, xproj);
    return;
  }
  const size_t lds = ((size_t)(cd.n + cd.F) + 4 * cd.F) * sizeof(float4);   // act, gbuf
  hipLaunchKernelGGL(k_lstm_fwd, dim3(grid), dim3(GMPC_THREADS), lds, s, Bc, cd, xseq, gates, cs, hp, hT, xproj);
}

void gmpc_launch_lstm_bwd(int Bc, const CriticDesc& cd, const float* gates, const float* cs,
                          const float* dhT, float* dz, float* dxseq, hipStream_t s) {
  const int grid = (Bc + 3) / 4;
  if (cd.F != 64) {
    hipLaunchKernelGGL(k_lstm_bwd_g, dim3(grid), dim3(GMPC_THREADS), (size_t)6 * cd.F * sizeof(float4), s, Bc,
                       cd, gates, cs, dhT, dz, dxseq);
    return;
  }
  const size_t lds = 2 * (size_t)(GMPC_THREADS + 128) * sizeof(float4);     // dzb, part
  hipLaunchKernelGGL(k_lstm_bwd, dim3(grid), dim3(GMPC_THREADS), lds, s, Bc, cd, gates, cs, dhT, dz, dxseq);
}
