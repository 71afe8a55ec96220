// The cross-entropy method solver (gmpc_cem_solve): trajax `cem` on this library's rollout.
// Per iteration: N control sequences per problem drawn around (mean, std), clamped to the bounds, rolled out and
// costed (k_cem_rollout); the E cheapest by (cost, index) refit mean and std (k_cem_update).  No noise and no sample
// is stored: a control is a pure function of (seed, iteration, problem, sample, step, control) -- cem_control, the
// one place a control is formed -- so the update regenerates the elites' controls instead of reading [B][N][T][m].
//
//   k_cem_rollout   one 256-thread workgroup per 32 samples of one problem, the whole horizon: the states stay in
//                   registers (the accumulator layout of dg_gemm), the layer inputs in LDS, every dynamics / cost layer
//                   on v_mfma_f32_16x16x4_f32 (dg_gemm, gmpc_dg_gemm.h), weights streamed from L2.
//   k_cem_update    one workgroup per problem: bitonic sort of 64-bit (cost, index) keys in LDS, then the elites'
//                   sums in rank order, one (step, control) per thread.
#include "gmpc_dg_gemm.h"
#include "gmpc_cem_sampler.h"

#include <cstring>

#define GMPC_CEM_ROWS 32          // samples per workgroup of the rollout (the two row halves of dg_gemm)
#define GMPC_CEM_MAX_N 4096       // samples per problem (the sort's keys: 32 KiB of LDS)

// ---- the rollout ----------------------------------------------------------------------------------------------
// Sum over the 8 lanes of a row's group (lanes 8 i .. 8 i + 7 of a wave), the same value in each: a fixed butterfly,
// so a row's sum does not depend on which row of which tile it is.
__device__ __forceinline__ float cem_row8_sum(float v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  return v;
}

// acc's rows into LDS columns 0 .. N-1 of the 32 operand rows (thread (wave, lane) holds D[4 kq + r][tile column])
template <typename F>
__device__ __forceinline__ void cem_store_tiles(float* Ab, const DgTiles& v, int N, int wave, int lane, F f) {
  const int l16 = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) {
    const int j = (wave + 4 * ci) * 16 + l16;
    if (j >= N) continue;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      Ab[(4 * kq + rr) * GMPC_DG_LDA + j] = f(v.p[ci][rr], j);
      Ab[(16 + 4 * kq + rr) * GMPC_DG_LDA + j] = f(v.q[ci][rr], j);
    }
  }
}

__global__ __launch_bounds__(GMPC_DG_THREADS) void k_cem_rollout(CemRollArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_cem[];
  float* Ab = reinterpret_cast<float*>(smem_cem);   // [32][GMPC_DG_LDA]: the layer inputs of the 32 sample rows
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, kq = lane >> 4;
  const int n = a.n, m = a.m, T = a.T, N = a.N;
  const int tiles = (N + GMPC_CEM_ROWS - 1) / GMPC_CEM_ROWS;
  const int b = blockIdx.x / tiles, s0 = (blockIdx.x - b * tiles) * GMPC_CEM_ROWS;
  const int rrow = tid >> 3, rc = tid & 7;   // the row whose sums this thread shares in, its lane of the row's 8
  const float w0 = sigmoidf_(a.mpc_w[0]), w1 = sigmoidf_(a.mpc_w[1]), w2 = sigmoidf_(a.mpc_w[2]);
  const float al = GMPC_ALPHA;
  const float* mean = a.mean + (size_t)b * T * m;
  const float* sd = a.sd + (size_t)b * T * m;
  // x_t of the 32 rows, in dg_gemm's accumulator layout: the output layer's tile of a thread is its tile of x
  DgTiles xs;
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) {
    const int j = (wave + 4 * ci) * 16 + l16;
    const float v = j < n ? a.x0[(size_t)b * n + j] : 0.f;
    xs.p[ci] = f32x4_t{v, v, v, v};
    xs.q[ci] = f32x4_t{v, v, v, v};
  }
  if (a.X)
    for (int j = tid; j < n; j += GMPC_DG_THREADS) a.X[(size_t)b * (T + 1) * n + j] = a.x0[(size_t)b * n + j];
  float csum = 0.f;   // the cost of row rrow so far (the same in its 8 lanes)
  DgTiles acc;
  for (int t = 0; t < T; ++t) {
    // ---- layer 0 input [x_t; u_t]
    cem_store_tiles(Ab, xs, n, wave, lane, [](float v, int) { return v; });
    for (int e = tid; e < GMPC_CEM_ROWS * m; e += GMPC_DG_THREADS) {
      const int i = e / m, j = e - i * m, s = s0 + i;
      const float lo = a.lo && !a.mean_row ? a.lo[j] : -INFINITY, hi = a.hi && !a.mean_row ? a.hi[j] : INFINITY;
      const float u = cem_control(a.rng, b, s, t, j, m, mean[t * m + j], a.mean_row ? 0.f : sd[t * m + j], lo, hi);
      Ab[i * GMPC_DG_LDA + n + j] = u;
      if (a.samples && s < N) a.samples[(((size_t)b * N + s) * T + t) * m + j] = u;
    }
    __syncthreads();
    // ---- stage cost of (x_t, u_t) against goal_t
    {
      const float* row = Ab + rrow * GMPC_DG_LDA;
      const float* g = a.goal + ((size_t)b * (T + 1) + t) * n;
      float su = 0.f, sx = 0.f;
      for (int j = rc; j < m; j += 8) su = fmaf(row[n + j], row[n + j], su);
      for (int j = rc; j < n; j += 8) {
        const float d = row[j] - g[j];
        sx = fmaf(d, d, sx);
      }
      su = cem_row8_sum(su);
      sx = cem_row8_sum(sx);
      csum += w0 * (sqrtf(su + al * al) - al) + w1 * (sqrtf(sx + al * al) - al);
    }
    // ---- x_{t+1} = x_t + MLP([x_t; u_t])
    for (int l = 0; l < a.dyn.L; ++l) {
      const int K = a.dyn.dims[l], Nl = a.dyn.dims[l + 1];
      dg_gemm(Ab, K, Nl, a.dyn.W[l], wave, lane, acc);
      __syncthreads();   // every wave has read its operand rows (and the stage cost its row)
      const float* bias = a.dyn.b[l];
      if (l < a.dyn.L - 1) {
        cem_store_tiles(Ab, acc, Nl, wave, lane, [bias](float v, int j) { return fmaxf(v + bias[j], 0.f); });
        __syncthreads();
      } else {
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
          const int j = (wave + 4 * ci) * 16 + l16;
          if (j >= n) continue;
          const float bj = bias[j];
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            xs.p[ci][rr] = (acc.p[ci][rr] + bj) + xs.p[ci][rr];
            xs.q[ci][rr] = (acc.q[ci][rr] + bj) + xs.q[ci][rr];
          }
          if (a.X && kq == 0) a.X[((size_t)b * (T + 1) + t + 1) * n + j] = xs.p[ci][0];   // row 0
        }
      }
    }
  }
  // ---- terminal cost w2 |MLP_c(x_T)|^2
  cem_store_tiles(Ab, xs, n, wave, lane, [](float v, int) { return v; });
  __syncthreads();
  for (int l = 0; l < a.cost.L; ++l) {
    const int K = a.cost.dims[l], Nl = a.cost.dims[l + 1];
    dg_gemm(Ab, K, Nl, a.cost.W[l], wave, lane, acc);
    __syncthreads();
    const float* bias = a.cost.b[l];
    if (l < a.cost.L - 1)
      cem_store_tiles(Ab, acc, Nl, wave, lane, [bias](float v, int j) { return fmaxf(v + bias[j], 0.f); });
    else
      cem_store_tiles(Ab, acc, Nl, wave, lane, [bias](float v, int j) { return v + bias[j]; });
    __syncthreads();
  }
  {
    const float* row = Ab + rrow * GMPC_DG_LDA;
    const int fout = a.cost.dims[a.cost.L];
    float sy = 0.f;
    for (int j = rc; j < fout; j += 8) sy = fmaf(row[j], row[j], sy);
    sy = cem_row8_sum(sy);
    csum += w2 * sy;
    if (rc == 0 && s0 + rrow < N) a.costs[(size_t)b * N + s0 + rrow] = csum;
  }
}

// ---- the update -----------------------------------------------------------------------------------------------
// Order-preserving bits of a cost (a NaN sorts as +inf, -0 as +0), then the sample index: ascending keys = the stable
// order
__device__ __forceinline__ unsigned long long cem_key(float c, int i) {
  uint32_t u = c != c ? 0x7F800000u : c == 0.f ? 0u : __float_as_uint(c);
  u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
  return ((unsigned long long)u << 32) | (uint32_t)i;
}

__global__ __launch_bounds__(GMPC_DG_THREADS) void k_cem_update(CemUpdArgs a, int P) {
  extern __shared__ __attribute__((aligned(16))) char smem_cu[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem_cu);   // [P], P the power of two >= N
  const int tid = threadIdx.x, b = blockIdx.x, N = a.N, E = a.E, T = a.T, m = a.m;
  for (int i = tid; i < P; i += GMPC_DG_THREADS)
    keys[i] = i < N ? cem_key(a.costs[(size_t)b * N + i], i) : ~0ull;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += GMPC_DG_THREADS) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned long long x = keys[i], y = keys[l];
          if ((x > y) == ((i & k) == 0)) { keys[i] = y; keys[l] = x; }
        }
      }
      __syncthreads();
    }
  if (a.elites)
    for (int r = tid; r < E; r += GMPC_DG_THREADS) a.elites[(size_t)b * E + r] = (int)(uint32_t)keys[r];
  // one (step, control) per thread: sums over the elites in rank order
  const float fE = (float)E, g = a.gamma, g1 = 1.f - a.gamma;
  for (int e = tid; e < T * m; e += GMPC_DG_THREADS) {
    const int t = e / m, j = e - t * m;
    const size_t o = (size_t)b * T * m + e;
    const float mu = a.mean[o], sg = a.sd[o];
    const float lo = a.lo ? a.lo[j] : -INFINITY, hi = a.hi ? a.hi[j] : INFINITY;
    float sum = 0.f;
    for (int r = 0; r < E; ++r) sum += cem_control(a.rng, b, (int)(uint32_t)keys[r], t, j, m, mu, sg, lo, hi);
    const float nm = sum / fE;
    float ss = 0.f;
    for (int r = 0; r < E; ++r) {
      const float d = cem_control(a.rng, b, (int)(uint32_t)keys[r], t, j, m, mu, sg, lo, hi) - nm;
      ss = __fadd_rn(ss, __fmul_rn(d, d));
    }
    const float ns = sqrtf(ss / fE);
    a.mean[o] = __fadd_rn(__fmul_rn(g, mu), __fmul_rn(g1, nm));
    a.sd[o] = __fadd_rn(__fmul_rn(g, sg), __fmul_rn(g1, ns));
  }
}

// Host-side launchers ---------------------------------------------------------------------------
int gmpc_launch_cem_rollout(const CemRollArgs& a, hipStream_t s) {
  for (int l = 0; l <= a.dyn.L; ++l)
    if (a.dyn.dims[l] > 256) return 1;
  for (int l = 0; l <= a.cost.L; ++l)
    if (a.cost.dims[l] > 256) return 1;
  if (a.n + a.m > 256 || a.N < 1 || a.N > GMPC_CEM_MAX_N) return 1;
  const int tiles = (a.N + GMPC_CEM_ROWS - 1) / GMPC_CEM_ROWS;
  const size_t lds = GMPC_CEM_ROWS * GMPC_DG_LDA * sizeof(float);
  hipLaunchKernelGGL(k_cem_rollout, dim3(a.B * tiles), dim3(GMPC_DG_THREADS), lds, s, a);
  return 0;
}

int gmpc_launch_cem_update(const CemUpdArgs& a, hipStream_t s) {
  if (a.N < 1 || a.N > GMPC_CEM_MAX_N || a.E < 1 || a.E > a.N) return 1;
  int P = 1;
  while (P < a.N) P <<= 1;
  hipLaunchKernelGGL(k_cem_update, dim3(a.B), dim3(GMPC_DG_THREADS), (size_t)P * sizeof(unsigned long long), s, a, P);
  return 0;
}
