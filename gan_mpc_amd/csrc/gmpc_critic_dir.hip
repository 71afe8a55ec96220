// Second-order VJP of the critic's scores (gmpc_critic_dir_vjp): the directional derivative sdot_b = <d score_b / d x_b,
// v_b> is the output of the tangent (forward-mode) critic run beside the primal one, and the call is the reverse sweep of
// that pair for a caller's delta on sdot.  No Hessian is formed.
//
// Notation (per unit and step): i, f, g, o the activated gates, z their pre-activations, c the cell, h the output; a dot
// marks a tangent (zd, cd, hd in the code), a bar an adjoint.  q' is the activation's derivative written in the activated
// value (q (1 - q), or 1 - g^2), q'' its derivative (q' (1 - 2 q), or -2 g g'); tc = tanh c.
//   forward   zd = v_t Wx + hd_{t-1} Wh (no bias),  qd = q' zd_q,  cd = fd c_ + f cd_ + id g + i gd,
//             hd = od tc + o tc' cd;  head: ad_{l+1} = mask_l o (ad_l W_l), sdot = ad_L  (the masks are the primal's)
//   backward  adjoints H, C (primal) and Hd, Cd (tangent); Hd_T = g_dir (tangent head)^T 1, the others start at zero:
//             od~ = Hd tc,  o~ = Hd tc' cd + H tc,  Cd += Hd o tc',  C += H o tc' + Hd (od tc' + o tc'' cd),
//             fd~ = Cd c_, id~ = Cd g, gd~ = Cd i,  f~ = Cd cd_ + C c_,  i~ = Cd gd + C g,  g~ = Cd id + C i,
//             C_ = C f + Cd fd,  Cd_ = Cd f,  z~_q = q~ q' + qd~ q'' zd_q,  zd~_q = qd~ q',
//             [x~_t ; H_] = [Wx ; Wh] z~,  [. ; Hd_] = [Wx ; Wh] zd~,
//             dW = sum [x ; h_]^T z~ + [v ; hd_]^T zd~,  db = sum z~;  head: dW_l = sum_b ad_l^T d_l, db_l = 0.
//
// One run-time-shape form for every critic with n + F <= 256 (F <= 128, head widths <= 256): the layout of k_lstm_fwd_g /
// k_lstm_bwd_g (gmpc_critic.hip).  A workgroup owns 4 sequences, held as float4 in LDS; primal and tangent lie side by
// side ([row][2] float4), so one pass over the weights -- streamed from L2, coalesced over the gate column -- feeds both
// matvecs (dense_rows<2>).  Gate columns, cell units and input rows are strided over the 256 threads; expf / tanhf
// activations.  The saves are this unit's own, [sequence][step] row-major: it reads nothing of the other critic kernels.
// The LSTM weight gradient is ONE GEMM A^T D over 2 Bc T1 rows with A = [[x, h_] ; [v, hd_]] (written by the forward
// sweep) and D = [z~ ; zd~] (written by the backward sweep); the bias gradient is the column sum of D's first half.
#include "gmpc_launch.h"

// act[k][0] = primal, act[k][1] = tangent: one float4 (4 sequences) each
__device__ __forceinline__ float* dir_f(float4* img, int k, int q) { return reinterpret_cast<float*>(img + 2 * k + q); }

__global__ __launch_bounds__(GMPC_THREADS) void k_dir_fwd(int Bc, CriticDesc cd, const float* __restrict__ xseq,
                                                          const float* __restrict__ vseq, DirSaves sv) {
  extern __shared__ __attribute__((aligned(16))) char smem_d[];
  const int tid = threadIdx.x;
  const int n = cd.n, F = cd.F, T1 = cd.T1, G4 = 4 * F, K = n + F;
  float4* act = reinterpret_cast<float4*>(smem_d);          // [n + F][2]: (x_t, v_t), then (h_{t-1}, hd_{t-1})
  float4* gbuf = act + 2 * K;                               // [4 F][2]: activated gates, their tangents
  float4* cst = gbuf + 2 * G4;                              // [F][2]: c, cd
  const int s0 = blockIdx.x * 4;
  const size_t R = (size_t)Bc * T1;
  int sq[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) sq[c] = min(s0 + c, Bc - 1);
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int e = tid; e < 2 * F; e += GMPC_THREADS) {
    act[2 * n + e] = zero4;
    cst[e] = zero4;
  }
  for (int t = 0; t < T1; ++t) {
    for (int e = tid; e < n * 4; e += GMPC_THREADS) {
      const int i = e >> 2, c = e & 3;
      const size_t at = ((size_t)sq[c] * T1 + t) * n + i;
      dir_f(act, i, 0)[c] = xseq[at];
      dir_f(act, i, 1)[c] = vseq[at];
    }
    __syncthreads();
    if (sv.A != nullptr) {                                  // operand rows [x_t, h_{t-1}] and [v_t, hd_{t-1}]
      for (int e = tid; e < K * 4; e += GMPC_THREADS) {
        const int c = e / K, k = e - c * K;
        if (s0 + c < Bc) {
          const size_t row = (size_t)(s0 + c) * T1 + t;
          sv.A[row * K + k] = dir_f(act, k, 0)[c];
          sv.A[(R + row) * K + k] = dir_f(act, k, 1)[c];
        }
      }
    }
    for (int j = tid; j < G4; j += GMPC_THREADS) {
      const float bj = cd.b[j];
      float4 acc[2] = {make_float4(bj, bj, bj, bj), zero4};
      dense_rows<2>(cd.Wcat, K, G4, j, act, acc);
      const bool is_g = j / F == 2;
      float q[4], qd[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float z = f4get(acc[0], c), zd = f4get(acc[1], c);
        q[c] = is_g ? tanhf(z) : sigmoidf_(z);
        qd[c] = (is_g ? 1.f - q[c] * q[c] : q[c] * (1.f - q[c])) * zd;
        if (s0 + c < Bc) {
          const size_t at = ((size_t)(s0 + c) * T1 + t) * G4 + j;
          sv.gates[at] = q[c];
          sv.zd[at] = zd;
        }
      }
      gbuf[2 * j] = make_float4(q[0], q[1], q[2], q[3]);
      gbuf[2 * j + 1] = make_float4(qd[0], qd[1], qd[2], qd[3]);
    }
    __syncthreads();
    for (int u = tid; u < F; u += GMPC_THREADS) {
      float cn[4], cdn[4], hn[4], hdn[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float ig = dir_f(gbuf, u, 0)[c], fg = dir_f(gbuf, F + u, 0)[c], gg = dir_f(gbuf, 2 * F + u, 0)[c],
                    og = dir_f(gbuf, 3 * F + u, 0)[c];
        const float id = dir_f(gbuf, u, 1)[c], fd = dir_f(gbuf, F + u, 1)[c], gd = dir_f(gbuf, 2 * F + u, 1)[c],
                    od = dir_f(gbuf, 3 * F + u, 1)[c];
        const float cp = dir_f(cst, u, 0)[c], cdp = dir_f(cst, u, 1)[c];
        cdn[c] = (fd * cp + fg * cdp) + (id * gg + ig * gd);
        cn[c] = fg * cp + ig * gg;
        const float tc = tanhf(cn[c]);
        hn[c] = og * tc;
        hdn[c] = od * tc + og * (1.f - tc * tc) * cdn[c];
        if (s0 + c < Bc) {
          const size_t at = ((size_t)(s0 + c) * T1 + t) * F + u;
          sv.cs[at] = cn[c];
          sv.cds[at] = cdn[c];
          if (t == T1 - 1) {
            sv.hT[(size_t)(s0 + c) * F + u] = hn[c];
            sv.hdT[(size_t)(s0 + c) * F + u] = hdn[c];
          }
        }
      }
      cst[2 * u] = make_float4(cn[0], cn[1], cn[2], cn[3]);
      cst[2 * u + 1] = make_float4(cdn[0], cdn[1], cdn[2], cdn[3]);
      act[2 * (n + u)] = make_float4(hn[0], hn[1], hn[2], hn[3]);
      act[2 * (n + u) + 1] = make_float4(hdn[0], hdn[1], hdn[2], hdn[3]);
    }
    __syncthreads();
  }
}

// The head on (h_T, hd_T): score and sdot, then (g_dir != null) the reverse of the TANGENT head for the delta g_dir on
// sdot: d_{L-1} = g_dir, d_l = mask_l o (d_{l+1} W_{l+1}^T), Hd_T = d_0 W_0^T.  No adjoint reaches the primal head: the
// masks are piecewise constant.  Thread j is neuron j of every layer (widths <= 256) in both directions, so the masks
// stay in registers.  Stored for the weight-gradient GEMMs in the layout `rows`: the tangent activations ad_l (acts) and
// the deltas d_l (dels).
__global__ __launch_bounds__(GMPC_THREADS) void k_dir_head(int Bc, CriticDesc cd, DirSaves sv,
                                                           const float* __restrict__ g_dir, float* __restrict__ score,
                                                           float* __restrict__ sdot, float* __restrict__ acts,
                                                           float* __restrict__ dels, MlpRows rows) {
  __shared__ __attribute__((aligned(16))) float4 img[2][2 * GMPC_THREADS];   // [buffer][k][primal, tangent]
  __shared__ __attribute__((aligned(16))) float4 dimg[2][GMPC_THREADS];      // [buffer][k] deltas
  __shared__ float red[4][8];
  __shared__ float dsc[4];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63;
  const int s0 = blockIdx.x * 4, stride = rows.stride;
  const MlpDesc& hd = cd.head;
  const int L = hd.L, F0 = hd.dims[0];
  const bool grad = g_dir != nullptr;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (tid < F0) {
    float a[4], ad[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int row = min(s0 + c, Bc - 1);
      a[c] = sv.hT[(size_t)row * F0 + tid];
      ad[c] = sv.hdT[(size_t)row * F0 + tid];
      if (grad && s0 + c < Bc) acts[(size_t)(s0 + c) * stride + rows.aoff[0] + tid] = ad[c];
    }
    img[0][2 * tid] = make_float4(a[0], a[1], a[2], a[3]);
    img[0][2 * tid + 1] = make_float4(ad[0], ad[1], ad[2], ad[3]);
  }
  __syncthreads();
  unsigned zmask[GMPC_MAX_LAYERS];       // bit c: relu open for sequence c of this thread's neuron
  int in = 0;
#pragma unroll
  for (int lay = 0; lay < GMPC_MAX_LAYERS; ++lay) {
    zmask[lay] = 0;
    if (lay < L - 1) {
      const int K = hd.dims[lay], N = hd.dims[lay + 1];
      if (tid < N) {
        const float bj = hd.b[lay][tid];
        float4 acc[2] = {make_float4(bj, bj, bj, bj), zero4};
        dense_rows<2>(hd.W[lay], K, N, tid, img[in], acc);
        float a[4], ad[4];
        unsigned zm = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float z = f4get(acc[0], c);
          const bool open = z > 0.f;
          zm |= open ? (1u << c) : 0u;
          a[c] = open ? z : 0.f;
          ad[c] = open ? f4get(acc[1], c) : 0.f;
          if (grad && s0 + c < Bc) acts[(size_t)(s0 + c) * stride + rows.aoff[lay + 1] + tid] = ad[c];
        }
        zmask[lay] = zm;
        img[in ^ 1][2 * tid] = make_float4(a[0], a[1], a[2], a[3]);
        img[in ^ 1][2 * tid + 1] = make_float4(ad[0], ad[1], ad[2], ad[3]);
      }
      in ^= 1;
      __syncthreads();
    }
  }
  // last layer: one output.  score = sum_k W[k] a[k] + b, sdot = sum_k W[k] ad[k]
  const int KL = hd.dims[L - 1];
  const float wl = tid < KL ? hd.W[L - 1][tid] : 0.f;
  {
    const float4 a4 = tid < KL ? img[in][2 * tid] : zero4, d4 = tid < KL ? img[in][2 * tid + 1] : zero4;
    const float pv[8] = {a4.x, a4.y, a4.z, a4.w, d4.x, d4.y, d4.z, d4.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float sm = wave_sum(wl * pv[e]);
      if (l == 0) red[w][e] = sm;
    }
  }
  __syncthreads();
  if (tid < 8) {
    const int c = tid & 3, row = s0 + c;
    const float v = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    if (row < Bc) {
      if (tid < 4) {
        if (score != nullptr) score[row] = v + hd.b[L - 1][0];
      } else {
        sdot[row] = v;
      }
    }
    if (tid >= 4) dsc[c] = (grad && row < Bc) ? g_dir[row] : 0.f;
  }
  if (!grad) return;
  __syncthreads();
  // delta of the last layer and the delta handed to the layer below
  {
    float r[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float ds = dsc[c];
      if (tid == 0 && s0 + c < Bc) dels[(size_t)(s0 + c) * stride + rows.doff[L - 1]] = ds;
      const bool open = L == 1 || ((zmask[(L + GMPC_MAX_LAYERS - 2) % GMPC_MAX_LAYERS] >> c) & 1u);
      r[c] = (tid < KL && open) ? wl * ds : 0.f;
    }
    if (L == 1) {
      // no hidden layer: Hd_T = W_last * g_dir
      if (tid < F0) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (s0 + c < Bc) sv.dhd[(size_t)(s0 + c) * F0 + tid] = r[c];
      }
      return;
    }
    dimg[0][tid] = make_float4(r[0], r[1], r[2], r[3]);
  }
  int din = 0;
  __syncthreads();
  // hidden layers, top down: dimg[din] holds d_lay ([dims[lay + 1]] x 4 sequences)
#pragma unroll
  for (int lay = GMPC_MAX_LAYERS - 2; lay >= 0; --lay) {
    if (lay < L - 1) {
      const int K = hd.dims[lay], N = hd.dims[lay + 1];
      if (tid < N) {
        const float4 v = dimg[din][tid];
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (s0 + c < Bc) dels[(size_t)(s0 + c) * stride + rows.doff[lay] + tid] = vv[c];
      }
      float4 acc[1] = {zero4};
      if (tid < K) dense_rows<1>(hd.WT[lay], N, K, tid, dimg[din], acc);
      if (lay > 0) {
        const unsigned zm = zmask[(lay + GMPC_MAX_LAYERS - 1) % GMPC_MAX_LAYERS];
        float r[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) r[c] = (tid < K && ((zm >> c) & 1u)) ? f4get(acc[0], c) : 0.f;
        dimg[din ^ 1][tid] = make_float4(r[0], r[1], r[2], r[3]);
        din ^= 1;
        __syncthreads();
      } else if (tid < K) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (s0 + c < Bc) sv.dhd[(size_t)(s0 + c) * F0 + tid] = f4get(acc[0], c);
      }
    }
  }
}

// The dual BPTT sweep.  D (optional): operand rows [z~ ; zd~] of the weight-gradient GEMM; dxseq (optional): x~.
__global__ __launch_bounds__(GMPC_THREADS) void k_dir_bwd(int Bc, CriticDesc cd, DirSaves sv, float* __restrict__ D,
                                                          float* __restrict__ dxseq) {
  extern __shared__ __attribute__((aligned(16))) char smem_d[];
  const int tid = threadIdx.x;
  const int n = cd.n, F = cd.F, T1 = cd.T1, G4 = 4 * F, K = n + F;
  float4* dzb = reinterpret_cast<float4*>(smem_d);          // [4 F][2]: z~, zd~
  float4* hb = dzb + 2 * G4;                                // [F][2]: H, Hd
  float4* cb = hb + 2 * F;                                  // [F][2]: C, Cd
  const int s0 = blockIdx.x * 4;
  const size_t R = (size_t)Bc * T1;
  int sq[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) sq[c] = min(s0 + c, Bc - 1);
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int u = tid; u < F; u += GMPC_THREADS) {
    // (a sequence past the batch starts from a zero adjoint: exact zeros all the way)
    float v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = s0 + c < Bc ? sv.dhd[(size_t)sq[c] * F + u] : 0.f;
    hb[2 * u] = zero4;
    hb[2 * u + 1] = make_float4(v[0], v[1], v[2], v[3]);
    cb[2 * u] = zero4;
    cb[2 * u + 1] = zero4;
  }
  __syncthreads();
  for (int t = T1 - 1; t >= 0; --t) {
    for (int u = tid; u < F; u += GMPC_THREADS) {
      float zb[4][4], zdb[4][4], Cn[4], Cdn[4];            // [gate][sequence]
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const size_t row = (size_t)sq[c] * T1 + t;
        const size_t gb = row * G4, ub = row * F + u;
        const float ig = sv.gates[gb + u], fg = sv.gates[gb + F + u], gg = sv.gates[gb + 2 * F + u],
                    og = sv.gates[gb + 3 * F + u];
        const float zi = sv.zd[gb + u], zf = sv.zd[gb + F + u], zg = sv.zd[gb + 2 * F + u], zo = sv.zd[gb + 3 * F + u];
        const float ct = sv.cs[ub], cdt = sv.cds[ub];
        const float cp = t > 0 ? sv.cs[ub - F] : 0.f, cdp = t > 0 ? sv.cds[ub - F] : 0.f;
        const float H = dir_f(hb, u, 0)[c], Hd = dir_f(hb, u, 1)[c];
        const float i1 = ig * (1.f - ig), f1 = fg * (1.f - fg), g1 = 1.f - gg * gg, o1 = og * (1.f - og);
        const float i2 = i1 * (1.f - 2.f * ig), f2 = f1 * (1.f - 2.f * fg), g2 = -2.f * gg * g1,
                    o2 = o1 * (1.f - 2.f * og);
        const float id = i1 * zi, fd = f1 * zf, gd = g1 * zg, od = o1 * zo;
        const float tc = tanhf(ct), tc1 = 1.f - tc * tc, tc2 = -2.f * tc * tc1;
        const float od_b = Hd * tc;
        const float o_b = Hd * tc1 * cdt + H * tc;
        const float Cd = dir_f(cb, u, 1)[c] + Hd * og * tc1;
        const float Cc = dir_f(cb, u, 0)[c] + (H * og * tc1 + Hd * (od * tc1 + og * tc2 * cdt));
        const float fd_b = Cd * cp, id_b = Cd * gg, gd_b = Cd * ig;
        const float f_b = Cd * cdp + Cc * cp;
        const float i_b = Cd * gd + Cc * gg;
        const float g_b = Cd * id + Cc * ig;
        Cn[c] = Cc * fg + Cd * fd;
        Cdn[c] = Cd * fg;
        zb[0][c] = i_b * i1 + id_b * i2 * zi;  zdb[0][c] = id_b * i1;
        zb[1][c] = f_b * f1 + fd_b * f2 * zf;  zdb[1][c] = fd_b * f1;
        zb[2][c] = g_b * g1 + gd_b * g2 * zg;  zdb[2][c] = gd_b * g1;
        zb[3][c] = o_b * o1 + od_b * o2 * zo;  zdb[3][c] = od_b * o1;
        if (D != nullptr && s0 + c < Bc) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            D[gb + q * F + u] = zb[q][c];
            D[R * G4 + gb + q * F + u] = zdb[q][c];
          }
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        dzb[2 * (q * F + u)] = make_float4(zb[q][0], zb[q][1], zb[q][2], zb[q][3]);
        dzb[2 * (q * F + u) + 1] = make_float4(zdb[q][0], zdb[q][1], zdb[q][2], zdb[q][3]);
      }
      cb[2 * u] = make_float4(Cn[0], Cn[1], Cn[2], Cn[3]);
      cb[2 * u + 1] = make_float4(Cdn[0], Cdn[1], Cdn[2], Cdn[3]);
    }
    __syncthreads();
    // [x~ ; H_{t-1}][k] = sum_j WcatT[j][k] z~[j], [. ; Hd_{t-1}][k] = sum_j WcatT[j][k] zd~[j]  (coalesced over k)
    for (int k = tid; k < K; k += GMPC_THREADS) {
      float4 acc[2] = {zero4, zero4};
      dense_rows<2>(cd.WcatT, G4, K, k, dzb, acc);
      if (k < n) {
        if (dxseq != nullptr) {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (s0 + c < Bc) dxseq[((size_t)(s0 + c) * T1 + t) * n + k] = f4get(acc[0], c);
        }
      } else {
        hb[2 * (k - n)] = acc[0];
        hb[2 * (k - n) + 1] = acc[1];
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
bool gmpc_dir_supported(const CriticDesc& cd) {
  return cd.n >= 1 && cd.F >= 1 && cd.F <= 128 && cd.n + cd.F <= GMPC_THREADS;
}

size_t gmpc_dir_save_floats(const CriticDesc& cd, int Bc) {
  return (size_t)Bc * cd.T1 * 10 * cd.F + (size_t)Bc * 3 * cd.F;
}

void gmpc_dir_bind_saves(const CriticDesc& cd, int Bc, float* save, DirSaves* sv) {
  const size_t R = (size_t)Bc * cd.T1, F = cd.F;
  sv->gates = save;
  sv->zd = sv->gates + R * 4 * F;
  sv->cs = sv->zd + R * 4 * F;
  sv->cds = sv->cs + R * F;
  sv->hT = sv->cds + R * F;
  sv->hdT = sv->hT + (size_t)Bc * F;
  sv->dhd = sv->hdT + (size_t)Bc * F;
  sv->A = nullptr;
}

void gmpc_launch_dir_fwd(int Bc, const CriticDesc& cd, const float* xseq, const float* vseq, const DirSaves& sv,
                         hipStream_t s) {
  const size_t lds = (2 * (size_t)(cd.n + cd.F) + 10 * (size_t)cd.F) * sizeof(float4);
  hipLaunchKernelGGL(k_dir_fwd, dim3((Bc + 3) / 4), dim3(GMPC_THREADS), lds, s, Bc, cd, xseq, vseq, sv);
}

void gmpc_launch_dir_head(int Bc, const CriticDesc& cd, const DirSaves& sv, const float* g_dir, float* score, float* sdot,
                          float* acts, float* dels, const MlpRows& rows, hipStream_t s) {
  hipLaunchKernelGGL(k_dir_head, dim3((Bc + 3) / 4), dim3(GMPC_THREADS), 0, s, Bc, cd, sv, g_dir, score, sdot, acts,
                     dels, rows);
}

void gmpc_launch_dir_bwd(int Bc, const CriticDesc& cd, const DirSaves& sv, float* D, float* dxseq, hipStream_t s) {
  const size_t lds = (size_t)12 * cd.F * sizeof(float4);
  hipLaunchKernelGGL(k_dir_bwd, dim3((Bc + 3) / 4), dim3(GMPC_THREADS), lds, s, Bc, cd, sv, D, dxseq);
}
