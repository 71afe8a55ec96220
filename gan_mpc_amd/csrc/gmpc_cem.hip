// The cross-entropy method solver (gmpc_cem_solve): trajax `cem` on this library's rollout.
// Per iteration: N control sequences per problem drawn around (mean, std), clamped to the bounds, rolled out and
// costed (k_sampled_rollout); the E cheapest by (cost, index) refit mean and std (k_cem_update).  No noise and no sample
// is stored: a control is a pure function of (seed, iteration, problem, sample, step, control) -- cem_control, the
// one place a control is formed -- so the update regenerates the elites' controls instead of reading [B][N][T][m].
//
//   k_sampled_rollout<CemDrawn, BF16, Ens>  (gmpc_cem_rollout.h) one 256-thread workgroup per 32
//                   samples of one problem, the whole horizon: the states stay in registers (the accumulator layout of
//                   dg_gemm), the layer inputs in LDS, every dynamics / cost layer on the matrix cores (dg_gemm,
//                   gmpc_dg_gemm.h), weights streamed from L2.  This file instantiates its eight forms over CEM's
//                   rows: fp32 or bf16 operands (gmpc_set_sampled_precision, section 23); one model, every member of
//                   a dynamics ensemble (gmpc_set_sampled_ensemble, section 24), particles that draw their member
//                   per step (gmpc_set_sampled_ensemble_mode, section 26) or the nominal model with a member's
//                   one-step disagreement beside it (gmpc_set_sampled_disagreement, section 28).  MPPI launches the
//                   same eight.
//   k_ens_reduce    one thread per (problem, row): the planes' costs summed in plane order, times 1 / Q, into the
//                   cost buffer the update kernels read (shared with gmpc_icem.hip)
//   k_ens_reduce_risk  the same thread for the other two aggregates of section 26: mean plus a multiple of the
//                   planes' spread, or the worst plane
//   k_cem_update    one workgroup per problem: bitonic sort of 64-bit (cost, index) keys in LDS, then the elites'
//                   sums in rank order, one (step, control) per thread.
#include "gmpc_cem_rollout.h"

#include <cstring>

// ---- the rollout ----------------------------------------------------------------------------------------------
// The controls of CEM's rows: every row is drawn (cem_control); with mean_row the rows are the mean itself
struct CemDrawn {
  using Args = CemRollArgs;
  static __host__ __device__ __forceinline__ const CemRollArgs& roll(const Args& a) { return a; }
  static __host__ __device__ __forceinline__ int rows(const Args& a) { return a.N; }
  static __host__ __device__ __forceinline__ int ldc(const Args& a) { return a.N; }
  static int plan(Args&, size_t, size_t*) { return 0; }     // nothing of its own to refuse, no LDS of its own

  const CemRollArgs& a;
  const float *mean, *sd;
  __device__ __forceinline__ CemDrawn(const Args& a_, char*) : a(a_), mean(nullptr), sd(nullptr) {}
  __device__ __forceinline__ void begin(int b, int, int) {
    mean = a.mean + (size_t)b * a.T * a.m;
    sd = a.sd + (size_t)b * a.T * a.m;
  }
  __device__ __forceinline__ float control(int b, int, int s, int t, int j) const {
    const int m = a.m;
    const float lo = a.lo && !a.mean_row ? a.lo[j] : -INFINITY, hi = a.hi && !a.mean_row ? a.hi[j] : INFINITY;
    return cem_control(a.rng, b, s, t, j, m, mean[t * m + j], a.mean_row ? 0.f : sd[t * m + j], lo, hi);
  }
  __device__ __forceinline__ void record(int b, int s, int t, int j, float u) const {
    const int N = a.N, T = a.T, m = a.m;
    if (a.samples && s < N) a.samples[(((size_t)b * N + s) * T + t) * m + j] = u;
  }
};

template __global__ void k_sampled_rollout<CemDrawn, false, CemOneModel>(CemRollArgs, CemOneModel);
template __global__ void k_sampled_rollout<CemDrawn, true, CemOneModel>(CemRollArgs, CemOneModel);
template __global__ void k_sampled_rollout<CemDrawn, false, CemMember>(CemRollArgs, CemMember);
template __global__ void k_sampled_rollout<CemDrawn, true, CemMember>(CemRollArgs, CemMember);
template __global__ void k_sampled_rollout<CemDrawn, false, CemParticle>(CemRollArgs, CemParticle);
template __global__ void k_sampled_rollout<CemDrawn, true, CemParticle>(CemRollArgs, CemParticle);
template __global__ void k_sampled_rollout<CemDrawn, false, CemDisagree>(CemRollArgs, CemDisagree);
template __global__ void k_sampled_rollout<CemDrawn, true, CemDisagree>(CemRollArgs, CemDisagree);

// The ensemble's cost of a row under GMPC_ENS_MEAN: the planes' costs part [P][B][ldc] (P: the planes, members or
// particles) summed in ascending plane order, times invP, into costs [B][ldc]; one thread per (problem, row), rows
// below `rows` only (the rollouts wrote exactly those)
__global__ __launch_bounds__(GMPC_THREADS) void k_ens_reduce(const float* __restrict__ part, int P, int B, int rows,
                                                             int ldc, float invP, float* __restrict__ costs) {
  const int i = blockIdx.x * GMPC_THREADS + threadIdx.x;
  if (i >= B * rows) return;
  const int b = i / rows, s = i - b * rows;
  const size_t o = (size_t)b * ldc + s, plane = (size_t)B * ldc;
  float sum = part[o];
  for (int p = 1; p < P; ++p) sum = __fadd_rn(sum, part[p * plane + o]);
  costs[o] = __fmul_rn(sum, invP);
}

// The risk-sensitive aggregates over the planes part [Q][B][ldc], the same thread per (problem,
// row) and every operation one IEEE fp32 operation in ascending plane order, so NumPy restates it bit for bit.
//   MAX false: mean = (((J_0 + J_1) + ...) + J_{Q-1}) * invQ, ss = (((0 + d_0 d_0) + d_1 d_1) + ...) with d_q = J_q -
//              mean, cost = mean + risk * sqrt(ss * invQ); a NaN plane makes the mean, and with it the cost, NaN
//   MAX true:  the largest plane, a NaN sticky: w = J_0; w = (J_q > w || J_q != J_q) ? J_q : w
// One operation each: the arithmetic is written out under `fp contract(off)` -- in this build __fmul_rn / __fadd_rn are
// the plain operators, which the compiler's default contraction fuses into v_fmac_f32 (one rounding instead of two),
// and __fsqrt_rn is the native v_sqrt_f32 (1 ulp) -- and the root is sqrtf, correctly rounded.
template <bool MAX>
__global__ __launch_bounds__(GMPC_THREADS) void k_ens_reduce_risk(const float* __restrict__ part, int Q, int B, int rows,
                                                                  int ldc, float invQ, float risk,
                                                                  float* __restrict__ costs) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * GMPC_THREADS + threadIdx.x;
  if (i >= B * rows) return;
  const int b = i / rows, s = i - b * rows;
  const size_t o = (size_t)b * ldc + s, plane = (size_t)B * ldc;
  if constexpr (MAX) {
    float w = part[o];
    for (int q = 1; q < Q; ++q) {
      const float J = part[q * plane + o];
      w = (J > w || J != J) ? J : w;
    }
    costs[o] = w;
  } else {
    float sum = part[o];
    for (int q = 1; q < Q; ++q) sum = sum + part[q * plane + o];
    const float mean = sum * invQ;
    float ss = 0.f;
    for (int q = 0; q < Q; ++q) {
      const float d = part[q * plane + o] - mean;
      const float dd = d * d;
      ss = ss + dd;
    }
    const float var = ss * invQ;
    const float rs = risk * sqrtf(var);
    costs[o] = mean + rs;
  }
}

// ---- the update -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GMPC_DG_THREADS) void k_cem_update(CemUpdArgs a, int P) {
  extern __shared__ __attribute__((aligned(16))) char smem_cu[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem_cu);   // [P], P the power of two >= N
  const int tid = threadIdx.x, b = blockIdx.x, N = a.N, E = a.E, T = a.T, m = a.m;
  for (int i = tid; i < P; i += GMPC_DG_THREADS)
    keys[i] = i < N ? cem_key(a.costs[(size_t)b * N + i], i) : ~0ull;
  __syncthreads();
  cem_sort_keys(keys, P, tid);
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
int gmpc_launch_sampled_rollout(const CemRollArgs& a, bool bf16, const CemEnsemble* ens, hipStream_t s) {
  return sampled_launch_rollout<CemDrawn>(a, bf16, ens, s);
}

void gmpc_launch_ens_reduce(const CemEnsemble& e, int B, int rows, int ldc, float* costs, hipStream_t s) {
  const int blocks = (int)(((size_t)B * rows + GMPC_THREADS - 1) / GMPC_THREADS);
  if (e.aggregate == GMPC_ENS_MEAN)
    hipLaunchKernelGGL(k_ens_reduce, dim3(blocks), dim3(GMPC_THREADS), 0, s, e.part, e.Q, B, rows, ldc, e.invQ, costs);
  else if (e.aggregate == GMPC_ENS_MEAN_STD)
    hipLaunchKernelGGL(k_ens_reduce_risk<false>, dim3(blocks), dim3(GMPC_THREADS), 0, s, e.part, e.Q, B, rows, ldc,
                       e.invQ, e.risk, costs);
  else
    hipLaunchKernelGGL(k_ens_reduce_risk<true>, dim3(blocks), dim3(GMPC_THREADS), 0, s, e.part, e.Q, B, rows, ldc,
                       e.invQ, e.risk, costs);
}

int gmpc_launch_cem_update(const CemUpdArgs& a, hipStream_t s) {
  if (a.N < 1 || a.N > GMPC_CEM_MAX_N || a.E < 1 || a.E > a.N) return 1;
  int P = 1;
  while (P < a.N) P <<= 1;
  hipLaunchKernelGGL(k_cem_update, dim3(a.B), dim3(GMPC_DG_THREADS), (size_t)P * sizeof(unsigned long long), s, a, P);
  return 0;
}
