// The cross-entropy method solver (gmpc_cem_solve): trajax `cem` on this library's rollout.
// Per iteration: N control sequences per problem drawn around (mean, std), clamped to the bounds, rolled out and
// costed (k_cem_rollout); the E cheapest by (cost, index) refit mean and std (k_cem_update).  No noise and no sample
// is stored: a control is a pure function of (seed, iteration, problem, sample, step, control) -- cem_control, the
// one place a control is formed -- so the update regenerates the elites' controls instead of reading [B][N][T][m].
//
//   k_cem_rollout   one 256-thread workgroup per 32 samples of one problem, the whole horizon: the states stay in
//                   registers (the accumulator layout of dg_gemm), the layer inputs in LDS, every dynamics / cost layer
//                   on v_mfma_f32_16x16x4_f32 (dg_gemm, gmpc_dg_gemm.h), weights streamed from L2.  Its body is
//                   cem_rollout_body (gmpc_cem_rollout.h), which k_icem_rollout (gmpc_icem.hip) shares.
//   k_cem_rollout_bf16  the same body with bf16 matrix operands (gmpc_set_sampled_precision):
//                   dg_gemm_bf16 on v_mfma_f32_16x16x32_bf16 over packed bf16 weight images, a bf16 operand block in
//                   LDS behind the fp32 one.
//   k_cem_rollout_ens, k_cem_rollout_ens_bf16  the same body under every member of a dynamics ensemble
//                   (gmpc_set_sampled_ensemble): blockIdx.y is the member, whose weights the
//                   workgroup reads and whose plane of the call workspace takes its costs
//   k_ens_reduce    one thread per (problem, row): the members' costs summed in member order, times 1 / P, into the
//                   cost buffer the update kernels read (shared with gmpc_icem.hip)
//   k_cem_update    one workgroup per problem: bitonic sort of 64-bit (cost, index) keys in LDS, then the elites'
//                   sums in rank order, one (step, control) per thread.
#include "gmpc_cem_rollout.h"

#include <cstring>

// ---- the rollout ----------------------------------------------------------------------------------------------
// The controls of CEM's rows: every row is drawn (cem_control); with mean_row the rows are the mean itself
struct CemDrawn {
  const CemRollArgs& a;
  const float *mean, *sd;
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

__global__ __launch_bounds__(GMPC_DG_THREADS) void k_cem_rollout(CemRollArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_cem[];
  float* Ab = reinterpret_cast<float*>(smem_cem);   // [32][GMPC_DG_LDA]: the layer inputs of the 32 sample rows
  CemDrawn src{a, nullptr, nullptr};
  cem_rollout_body<false>(a, a.N, a.N, Ab, nullptr, src);
}

// The same rows with bf16 matrix operands: a.dyn.W / a.cost.W are the packed bf16 images
__global__ __launch_bounds__(GMPC_DG_THREADS) void k_cem_rollout_bf16(CemRollArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_cem16[];
  float* Ab = reinterpret_cast<float*>(smem_cem16);   // [32][GMPC_DG_LDA] fp32: [x_t; u_t], the last cost output
  __bf16* Hb = reinterpret_cast<__bf16*>(Ab + GMPC_CEM_ROWS * GMPC_DG_LDA);   // [32][GMPC_DG_LDH]: the layer inputs
  CemDrawn src{a, nullptr, nullptr};
  cem_rollout_body<true>(a, a.N, a.N, Ab, Hb, src);
}

// The same rows under every member of a dynamics ensemble (gmpc_set_sampled_ensemble): the grid's
// second dimension is the member, whose weights the workgroup reads and whose plane of e.part it writes
__global__ __launch_bounds__(GMPC_DG_THREADS) void k_cem_rollout_ens(CemRollArgs a, CemMember e) {
  extern __shared__ __attribute__((aligned(16))) char smem_cem_e[];
  float* Ab = reinterpret_cast<float*>(smem_cem_e);
  CemDrawn src{a, nullptr, nullptr};
  cem_rollout_body<false>(a, a.N, a.N, Ab, nullptr, src, e);
}

__global__ __launch_bounds__(GMPC_DG_THREADS) void k_cem_rollout_ens_bf16(CemRollArgs a, CemMember e) {
  extern __shared__ __attribute__((aligned(16))) char smem_cem_e16[];
  float* Ab = reinterpret_cast<float*>(smem_cem_e16);
  __bf16* Hb = reinterpret_cast<__bf16*>(Ab + GMPC_CEM_ROWS * GMPC_DG_LDA);
  CemDrawn src{a, nullptr, nullptr};
  cem_rollout_body<true>(a, a.N, a.N, Ab, Hb, src, e);
}

// The ensemble's cost of a row: the members' costs part [P][B][ldc] summed in ascending member order, times invP, into
// costs [B][ldc]; one thread per (problem, row), rows below `rows` only (the rollouts wrote exactly those)
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
static int cem_rollout_covered(const CemRollArgs& a) {
  for (int l = 0; l <= a.dyn.L; ++l)
    if (a.dyn.dims[l] > 256) return 0;
  for (int l = 0; l <= a.cost.L; ++l)
    if (a.cost.dims[l] > 256) return 0;
  return !(a.n + a.m > 256 || a.N < 1 || a.N > GMPC_CEM_MAX_N);
}

int gmpc_launch_cem_rollout(const CemRollArgs& a, hipStream_t s) {
  if (!cem_rollout_covered(a)) return 1;
  const int tiles = (a.N + GMPC_CEM_ROWS - 1) / GMPC_CEM_ROWS;
  const size_t lds = GMPC_CEM_ROWS * GMPC_DG_LDA * sizeof(float);
  hipLaunchKernelGGL(k_cem_rollout, dim3(a.B * tiles), dim3(GMPC_DG_THREADS), lds, s, a);
  return 0;
}

int gmpc_launch_cem_rollout_bf16(const CemRollArgs& a, hipStream_t s) {
  if (!cem_rollout_covered(a) || a.mean_row) return 1;     // (the returned sequence's rollout is the fp32 kernel's)
  const int tiles = (a.N + GMPC_CEM_ROWS - 1) / GMPC_CEM_ROWS;
  hipLaunchKernelGGL(k_cem_rollout_bf16, dim3(a.B * tiles), dim3(GMPC_DG_THREADS), GMPC_CEM_LDS16, s, a);
  return 0;
}

void gmpc_launch_ens_reduce(const CemEnsemble& e, int B, int rows, int ldc, float* costs, hipStream_t s) {
  const int blocks = (int)(((size_t)B * rows + GMPC_THREADS - 1) / GMPC_THREADS);
  hipLaunchKernelGGL(k_ens_reduce, dim3(blocks), dim3(GMPC_THREADS), 0, s, e.part, e.P, B, rows, ldc, e.invP, costs);
}

// a.dyn: member 0 (bf16: its images); two launches, the members' rollouts and the reduce into a.costs
int gmpc_launch_cem_rollout_ens(const CemRollArgs& a, const CemEnsemble& e, bool bf16, hipStream_t s) {
  if (!cem_rollout_covered(a) || a.mean_row || a.X || e.P < 1 || e.P > GMPC_MAX_ENSEMBLE || !e.part) return 1;
  const int tiles = (a.N + GMPC_CEM_ROWS - 1) / GMPC_CEM_ROWS;
  const CemMember mb{e.wstride, e.bstride, (size_t)a.B * a.N, e.part};
  if (bf16)
    hipLaunchKernelGGL(k_cem_rollout_ens_bf16, dim3(a.B * tiles, e.P), dim3(GMPC_DG_THREADS), GMPC_CEM_LDS16, s, a, mb);
  else
    hipLaunchKernelGGL(k_cem_rollout_ens, dim3(a.B * tiles, e.P), dim3(GMPC_DG_THREADS), GMPC_CEM_LDS32, s, a, mb);
  gmpc_launch_ens_reduce(e, a.B, a.N, a.N, a.costs, s);
  return 0;
}

int gmpc_launch_cem_update(const CemUpdArgs& a, hipStream_t s) {
  if (a.N < 1 || a.N > GMPC_CEM_MAX_N || a.E < 1 || a.E > a.N) return 1;
  int P = 1;
  while (P < a.N) P <<= 1;
  hipLaunchKernelGGL(k_cem_update, dim3(a.B), dim3(GMPC_DG_THREADS), (size_t)P * sizeof(unsigned long long), s, a, P);
  return 0;
}
