// Dynamics-model regression for an ensemble of relu-MLP dynamics on the matrix cores (gmpc_dynamics_ensemble_loss_grad;
// DESIGN.md section 25): the multi-step prediction loss of gmpc_dynfit.hip and its sweep back through time, for P
// members at once.
//
//   k_dynfit_rows       grid (ceil(B / 32), P): one workgroup owns 32 sequences of one member for the forward sweep and
//                       the backward sweep over the S steps.  The 32 sequences are the 32 operand rows of dg_gemm (both
//                       halves carry sequences; dfr_gemm below runs dg_gemm's products); the state, the future's adjoint and the step's cotangent stay in
//                       registers in dg_gemm's accumulator layout, so the output tile of a thread is its tile of x.
//                       Layer inputs and output deltas go to the member's acts / dels rows (row b S + t), the operands
//                       of the weight-gradient GEMMs; the residual pred_t - y_t waits in the delta_L columns of its row
//                       between the two sweeps.  The last tile's workgroup zeroes the member's pad rows.
//   k_dynfit_transpose  W_l -> W_l^T of every layer of every member, one launch (the members change at every optimiser
//                       step, so the transposes are built per call).
//   k_dynfit_loss_sum   loss_sum[p] = the B per-sequence losses of member p, in a fixed order.
// No atomics, no scratch, no state: every float a kernel reads was written earlier in the same call.
#include "gmpc_dg_gemm.h"

#include <cstring>

#define GMPC_DFR_ROWS 32         // sequences per workgroup
#define GMPC_DFR_RED 65          // row stride of the loss partials (64 column slots + 1)

// dg_gemm -- the same operands, tiles and accumulator layout, the same products in the same order on every accumulator
// -- for a workgroup that runs 8 S GEMMs one behind the other at one wave per SIMD, where the wait for a k-step's
// weights, not the matrix pipe, sets dg_gemm's time.  The wave's NT column tiles are a template parameter (a uniform
// switch, as in dg_gemm_bf16), so the loop body has no branch: every load is unconditional (off-range columns and k are
// clamped to valid addresses and their products discarded or zeroed by a select), and the 4 NT weights of the next
// block of 16 k are requested before this block's 8 NT products issue.  The fence stands at the end of every turn, on
// the accumulation half of the register file, which is where hipcc keeps this kernel's accumulators.
template <int NT>
__device__ __forceinline__ void dfr_gemm_tiles(const float* pa, const float* qa, const float* __restrict__ Wg, int K,
                                               int N, int kq, const int (&col)[4], DgTiles& acc) {
  const float* wc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) wc[i] = Wg + (size_t)kq * N + col[i];
  const int Kb = K & ~15;
  float w[4][NT], wn[4][NT];
  if (Kb > 0) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < NT; ++i) w[s][i] = wc[i][(size_t)(4 * s) * N];
  }
  int k0 = 0;
  for (; k0 < Kb; k0 += 16) {
    const int kn = k0 + 16 < Kb ? k0 + 16 : k0;     // (the last block asks for its own weights again)
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < NT; ++i) wn[s][i] = wc[i][(size_t)(kn + 4 * s) * N];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float a0 = pa[k0 + 4 * s], b0 = qa[k0 + 4 * s];
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        acc.p[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, w[s][i], acc.p[i], 0, 0, 0);
        acc.q[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(b0, w[s][i], acc.q[i], 0, 0, 0);
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < NT; ++i) w[s][i] = wn[s][i];
    if constexpr (NT == 4)
      mfma_fence<true>(acc.p[0], acc.q[0], acc.p[1], acc.q[1], acc.p[2], acc.q[2], acc.p[3], acc.q[3]);
    if constexpr (NT == 3) mfma_fence<true>(acc.p[0], acc.q[0], acc.p[1], acc.q[1], acc.p[2], acc.q[2]);
    if constexpr (NT == 2) mfma_fence<true>(acc.p[0], acc.q[0], acc.p[1], acc.q[1]);
    if constexpr (NT == 1) mfma_fence<true>(acc.p[0], acc.q[0]);
  }
  for (; k0 < K; k0 += 4) {
    const bool kin = k0 + kq < K;
    const int kc = kin ? k0 : K - 1 - kq;           // this lane's row K - 1: a valid address, its product zeroed
    float w0[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const float v = wc[i][(long)kc * N];
      w0[i] = kin ? v : 0.f;
    }
    const float av = pa[k0], bv = qa[k0];           // (k0 + kq < GMPC_DG_LDA: inside the row)
    const float a0 = kin ? av : 0.f, b0 = kin ? bv : 0.f;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      acc.p[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, w0[i], acc.p[i], 0, 0, 0);
      acc.q[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(b0, w0[i], acc.q[i], 0, 0, 0);
    }
    if constexpr (NT == 4)
      mfma_fence<true>(acc.p[0], acc.q[0], acc.p[1], acc.q[1], acc.p[2], acc.q[2], acc.p[3], acc.q[3]);
    if constexpr (NT == 3) mfma_fence<true>(acc.p[0], acc.q[0], acc.p[1], acc.q[1], acc.p[2], acc.q[2]);
    if constexpr (NT == 2) mfma_fence<true>(acc.p[0], acc.q[0], acc.p[1], acc.q[1]);
    if constexpr (NT == 1) mfma_fence<true>(acc.p[0], acc.q[0]);
  }
}

__device__ __forceinline__ void dfr_gemm(const float* A, int K, int N, const float* __restrict__ Wg, int wave, int lane,
                                         DgTiles& acc) {
  const int l16 = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    acc.p[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    acc.q[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  const int wu = __builtin_amdgcn_readfirstlane(wave), nct = (N + 15) >> 4;
  const int nt = nct > wu ? (nct - wu + 3) >> 2 : 0;      // the wave's tiles wave, wave + 4, ...: the first nt of four
  int col[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = (wu + 4 * i) * 16 + l16;
    col[i] = j < N ? j : N - 1;
  }
  const float* pa = A + l16 * GMPC_DG_LDA + kq;
  const float* qa = A + (16 + l16) * GMPC_DG_LDA + kq;
  switch (nt) {
    case 4: dfr_gemm_tiles<4>(pa, qa, Wg, K, N, kq, col, acc); break;
    case 3: dfr_gemm_tiles<3>(pa, qa, Wg, K, N, kq, col, acc); break;
    case 2: dfr_gemm_tiles<2>(pa, qa, Wg, K, N, kq, col, acc); break;
    case 1: dfr_gemm_tiles<1>(pa, qa, Wg, K, N, kq, col, acc); break;
    default: break;     // (no tile: the zeros above)
  }
}

__global__ __launch_bounds__(GMPC_DG_THREADS) void k_dynfit_rows(DynFitRowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_dfr[];
  float* Ab = reinterpret_cast<float*>(smem_dfr);      // [32][GMPC_DG_LDA] layer inputs (forward) / deltas (backward)
  float* disc = Ab + 32 * GMPC_DG_LDA;                 // [S]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, kq = lane >> 4;
  const int n = a.n, m = a.m, nm = n + m, L = a.dyn.L, S = a.S, B = a.B;
  const int s0 = blockIdx.x * GMPC_DFR_ROWS;
  const size_t p = blockIdx.y, st = a.lay.stride;
  float* acts = a.acts + p * a.rstride;
  float* dels = a.dels + p * a.rstride;
  const int* rows = a.rows ? a.rows + p * B : nullptr;
  const int dL = a.lay.doff[L - 1];
  if (tid == 0) {
    float d = 1.f;
    for (int t = 0; t < S; ++t) { disc[t] = d; d *= a.gamma; }
  }
  // the pad rows behind the member's B S rows (read, not used, by the weight-gradient GEMMs)
  if (blockIdx.x == gridDim.x - 1) {
    const size_t o = (size_t)B * S * st;
    for (size_t e = tid; e < GMPC_WGRAD_PAD * st; e += GMPC_DG_THREADS) {
      acts[o + e] = 0.f;
      dels[o + e] = 0.f;
    }
  }
  // The thread's 8 sequences in the accumulator layout: half h (0: p, 1: q), register rr -> operand row 16 h + 4 kq +
  // rr.  seq: the dataset row (of a clamped sequence past B), row: the first acts / dels row (B S rows: an int), ok:
  // inside the batch.
  int seq[2][4], row[2][4];
  bool ok[2][4];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int b = s0 + 16 * h + 4 * kq + rr, bc = b < B ? b : B - 1;
      ok[h][rr] = b < B;
      seq[h][rr] = rows ? rows[bc] : bc;
      row[h][rr] = bc * S;
    }
  __syncthreads();
  DgTiles xs, acc;
  float lacc[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  // ---------------------------------------------------------------- forward sweep
  for (int t = 0; t < S; ++t) {
    if (t == 0 || a.teacher_forcing) {
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) {
        const int j = (wave + 4 * ci) * 16 + l16;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          xs.p[ci][rr] = j < n ? a.xseq[((size_t)seq[0][rr] * S + t) * n + j] : 0.f;
          xs.q[ci][rr] = j < n ? a.xseq[((size_t)seq[1][rr] * S + t) * n + j] : 0.f;
        }
      }
    }
    // ---- layer 0 input [x_in_t; u_t]
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) {
      const int j = (wave + 4 * ci) * 16 + l16;
      if (j >= n) continue;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int i = 4 * kq + rr;
        Ab[i * GMPC_DG_LDA + j] = xs.p[ci][rr];
        Ab[(16 + i) * GMPC_DG_LDA + j] = xs.q[ci][rr];
        if (ok[0][rr]) acts[(size_t)(row[0][rr] + t) * st + j] = xs.p[ci][rr];
        if (ok[1][rr]) acts[(size_t)(row[1][rr] + t) * st + j] = xs.q[ci][rr];
      }
    }
    for (int e = tid; e < GMPC_DFR_ROWS * m; e += GMPC_DG_THREADS) {
      const int i = e / m, j = e - i * m, b = s0 + i, bc = b < B ? b : B - 1;
      const float u = a.useq[((size_t)(rows ? rows[bc] : bc) * S + t) * m + j];
      Ab[i * GMPC_DG_LDA + n + j] = u;
      if (b < B) acts[((size_t)b * S + t) * st + n + j] = u;
    }
    __syncthreads();
    for (int l = 0; l < L; ++l) {
      const int K = a.dyn.dims[l], N = a.dyn.dims[l + 1];
      dfr_gemm(Ab, K, N, a.dyn.W[l] + p * a.mstride, wave, lane, acc);
      __syncthreads();   // every wave has read its operand rows
      const float* bias = a.dyn.b[l] + p * a.mstride;
      if (l < L - 1) {
        const int ao = a.lay.aoff[l + 1];
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
          const int j = (wave + 4 * ci) * 16 + l16;
          if (j >= N) continue;
          const float bj = bias[j];
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const int i = 4 * kq + rr;
            const float vp = fmaxf(acc.p[ci][rr] + bj, 0.f), vq = fmaxf(acc.q[ci][rr] + bj, 0.f);
            Ab[i * GMPC_DG_LDA + j] = vp;
            Ab[(16 + i) * GMPC_DG_LDA + j] = vq;
            if (ok[0][rr]) acts[(size_t)(row[0][rr] + t) * st + ao + j] = vp;
            if (ok[1][rr]) acts[(size_t)(row[1][rr] + t) * st + ao + j] = vq;
          }
        }
        __syncthreads();
      } else {
        // pred_t = x_in_t + MLP: the residual against y_t waits in the delta_L columns for the backward sweep
        const float w = disc[t];
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
          const int j = (wave + 4 * ci) * 16 + l16;
          if (j >= n) continue;
          const float bj = bias[j];
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const float vp = (acc.p[ci][rr] + bj) + xs.p[ci][rr], vq = (acc.q[ci][rr] + bj) + xs.q[ci][rr];
            const float dp = vp - a.yseq[((size_t)seq[0][rr] * S + t) * n + j];
            const float dq = vq - a.yseq[((size_t)seq[1][rr] * S + t) * n + j];
            lacc[0][rr] = fmaf(w * dp, dp, lacc[0][rr]);
            lacc[1][rr] = fmaf(w * dq, dq, lacc[1][rr]);
            if (ok[0][rr]) dels[(size_t)(row[0][rr] + t) * st + dL + j] = dp;
            if (ok[1][rr]) dels[(size_t)(row[1][rr] + t) * st + dL + j] = dq;
            xs.p[ci][rr] = vp;      // the next step's input when not teacher-forced
            xs.q[ci][rr] = vq;
          }
        }
      }
    }
  }
  // ---- per-sequence loss: the thread's columns (above), then the 64 column slots of a row in order
  {
    float* red = Ab;     // [32][GMPC_DFR_RED] (every wave is past the last product's barrier)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int i = 4 * kq + rr;
      red[i * GMPC_DFR_RED + wave * 16 + l16] = lacc[0][rr];
      red[(16 + i) * GMPC_DFR_RED + wave * 16 + l16] = lacc[1][rr];
    }
    __syncthreads();
    if (tid < GMPC_DFR_ROWS && s0 + tid < B) {
      float sum = 0.f;
      for (int c = 0; c < 64; ++c) sum += red[tid * GMPC_DFR_RED + c];
      a.loss[p * B + s0 + tid] = sum;
    }
    __syncthreads();
  }
  // ---------------------------------------------------------------- backward sweep
  DgTiles lam, gs;     // dL/d pred_t from the future; d loss / d pred_t of the current step
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) {
    lam.p[ci] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    lam.q[ci] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  for (int t = S - 1; t >= 0; --t) {
    const float w2 = 2.f * disc[t];
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) {
      const int j = (wave + 4 * ci) * 16 + l16;
      if (j >= n) continue;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int i = 4 * kq + rr;
        const size_t op = (size_t)(row[0][rr] + t) * st + dL + j, oq = (size_t)(row[1][rr] + t) * st + dL + j;
        const float gp = ok[0][rr] ? w2 * dels[op] + lam.p[ci][rr] : 0.f;     // (this thread's own store)
        const float gq = ok[1][rr] ? w2 * dels[oq] + lam.q[ci][rr] : 0.f;
        if (ok[0][rr]) dels[op] = gp;
        if (ok[1][rr]) dels[oq] = gq;
        gs.p[ci][rr] = gp;
        gs.q[ci][rr] = gq;
        Ab[i * GMPC_DG_LDA + j] = gp;
        Ab[(16 + i) * GMPC_DG_LDA + j] = gq;
      }
    }
    __syncthreads();
    for (int l = L - 1; l >= 1; --l) {
      const int K = a.dyn.dims[l + 1], N = a.dyn.dims[l];      // d_l = relu'(a_l) . (d_{l+1} W_l^T)
      dfr_gemm(Ab, K, N, a.dyn.WT[l] + p * a.mstride, wave, lane, acc);
      __syncthreads();
      const int ao = a.lay.aoff[l], dof = a.lay.doff[l - 1];
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) {
        const int j = (wave + 4 * ci) * 16 + l16;
        if (j >= N) continue;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int i = 4 * kq + rr;
          const size_t rp = (size_t)(row[0][rr] + t) * st, rq = (size_t)(row[1][rr] + t) * st;
          const float dp = ok[0][rr] && acts[rp + ao + j] > 0.f ? acc.p[ci][rr] : 0.f;   // (its own store again)
          const float dq = ok[1][rr] && acts[rq + ao + j] > 0.f ? acc.q[ci][rr] : 0.f;
          Ab[i * GMPC_DG_LDA + j] = dp;
          Ab[(16 + i) * GMPC_DG_LDA + j] = dq;
          if (ok[0][rr]) dels[rp + dof + j] = dp;
          if (ok[1][rr]) dels[rq + dof + j] = dq;
        }
      }
      __syncthreads();
    }
    if (!a.teacher_forcing && t > 0) {
      // lam_{t-1} = (d_1 W_0^T)[:n] + g_t: the input's x columns, and the residual's pass-through
      dfr_gemm(Ab, a.dyn.dims[1], nm, a.dyn.WT[0] + p * a.mstride, wave, lane, acc);
      __syncthreads();
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) {
        const int j = (wave + 4 * ci) * 16 + l16;
        if (j >= n) continue;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          lam.p[ci][rr] = acc.p[ci][rr] + gs.p[ci][rr];
          lam.q[ci][rr] = acc.q[ci][rr] + gs.q[ci][rr];
        }
      }
    }
  }
}

// every layer of every member: in [K][N] -> out [N][K]; grid (ceil(max K N / 256), L, P)
__global__ __launch_bounds__(256) void k_dynfit_transpose(MlpDesc d, size_t mstride, float* WT0) {
  const int l = blockIdx.y, K = d.dims[l], N = d.dims[l + 1];
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= K * N) return;
  const int c = e / K, r = e - c * K;      // out element (c, r): consecutive threads write consecutive floats
  const size_t off = blockIdx.z * mstride;
  const float* in = d.W[l] + off;
  float* out = WT0 + (d.WT[l] - d.WT[0]) + off;
  out[e] = in[(size_t)r * N + c];
}

// loss_sum[p] = sum_b loss[p][b]: thread-strided partials, the waves' sums, then the 4 wave sums in order
__global__ __launch_bounds__(256) void k_dynfit_loss_sum(int B, const float* loss, float* loss_sum) {
  __shared__ float red[4];
  const float* v = loss + (size_t)blockIdx.x * B;
  float s = 0.f;
  for (int e = threadIdx.x; e < B; e += 256) s += v[e];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) loss_sum[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// Host side -----------------------------------------------------------------------------------------------------------
size_t gmpc_dynfit_rows_lds(int S) { return (32 * (size_t)GMPC_DG_LDA + (size_t)S) * sizeof(float); }

void gmpc_launch_dynfit_transpose(const MlpDesc& d, size_t mstride, int P, float* WT0, hipStream_t s) {
  int kn = 1;
  for (int l = 0; l < d.L; ++l) kn = d.dims[l] * d.dims[l + 1] > kn ? d.dims[l] * d.dims[l + 1] : kn;
  hipLaunchKernelGGL(k_dynfit_transpose, dim3((kn + 255) / 256, d.L, P), dim3(256), 0, s, d, mstride, WT0);
}

int gmpc_launch_dynfit_rows(const DynFitRowsArgs& a, int P, float* WT0, float* loss_sum, hipStream_t s) {
  const MlpDesc& d = a.dyn;
  int kn = 1;
  for (int l = 0; l <= d.L; ++l)
    if (d.dims[l] > GMPC_SAMPLED_MAX_WIDTH) return 1;
  if (a.n + a.m > GMPC_SAMPLED_MAX_WIDTH || P < 1 || P > GMPC_MAX_ENSEMBLE) return 1;
  const size_t lds = gmpc_dynfit_rows_lds(a.S);
  if (lds > 64 * 1024) return 1;
  for (int l = 0; l < d.L; ++l) kn = d.dims[l] * d.dims[l + 1] > kn ? d.dims[l] * d.dims[l + 1] : kn;
  hipLaunchKernelGGL(k_dynfit_transpose, dim3((kn + 255) / 256, d.L, P), dim3(256), 0, s, d, a.mstride, WT0);
  hipLaunchKernelGGL(k_dynfit_rows, dim3((a.B + GMPC_DFR_ROWS - 1) / GMPC_DFR_ROWS, P), dim3(GMPC_DG_THREADS), lds, s,
                     a);
  hipLaunchKernelGGL(k_dynfit_loss_sum, dim3(P), dim3(256), 0, s, a.B, a.loss, loss_sum);
  return 0;
}
