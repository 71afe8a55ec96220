// The sample-efficient cross-entropy method (gmpc_icem_solve; Pinneri et al., CoRL 2020) on the
// sampled rollout of the cross-entropy method.  Per iteration a pool of rows per problem -- fresh samples with
// power-law ("coloured") noise along the horizon, the rows kept from the iteration before, in the last iteration the
// mean itself -- is rolled out and costed (k_sampled_rollout over IcemDrawn: CEM's rollout over another source of
// controls); the E cheapest by (cost, row) refit mean and std, the cheapest of them become the next kept rows, and
// the best row seen so far is remembered (k_icem_update).  As in gmpc_cem.hip no noise and no sample is stored: a
// fresh control is a pure function of (seed, iteration, problem, sample, step, control) -- icem_control, the one
// place a pool row's control is formed -- and the update regenerates the elites' controls.
//
//   k_sampled_rollout<IcemDrawn, BF16, Ens>  (gmpc_cem_rollout.h) the rollout kernel over the pool's rows, eight forms
//                   as in gmpc_cem.hip: fp32 or bf16 operands; one model, every member of a dynamics ensemble,
//                   particles that draw their member per step, or the nominal model with a member's one-step
//                   disagreement beside it.  The
//                   coloured sum of a control needs the T normals of its (row, control): formed once per tile in LDS
//                   behind the operand blocks where 32 m T floats fit there (zlds), regenerated per element otherwise
//                   -- the same sum in the same order either way.
//   k_icem_update   one workgroup per problem: the sort of k_cem_update over the pool's rows, then the elites' sums in
//                   rank order (for T m < 256 by the whole workgroup, in blocks of elites staged in LDS: the same
//                   sums), the kept rows, the best row and the returned sequence.
#include "gmpc_cem_rollout.h"

#include <cstring>

#define GMPC_ICEM_STAGE_FLOATS 4096   // k_icem_update's staged controls (16 KiB of LDS behind the keys)

// ---- the controls of a pool row -------------------------------------------------------------------------------
// zt_t = cw_0 z_0 + sum_{1 <= k, 2k < T} cw_k (z_{2k-1} cos(2 pi k t / T) + z_{2k} sin(2 pi k t / T))
//        + [T even] cw_{T/2} z_{T-1} (-1)^t:  the orthonormal real DFT basis under power-law weights.  k ascending, the
// angle as cospi / sinpi of 2 ((k t) mod T) / T with the product reduced in integers, so no rounding of k t reaches
// it.  z(k): the k-th normal of the (row, control).
template <typename Z>
__device__ __forceinline__ float icem_colour(const float* cw, int T, int t, Z z) {
  float acc = __fmul_rn(cw[0], z(0));
  int q = 0, k = 1;
  for (; 2 * k < T; ++k) {
    q += t;
    if (q >= T) q -= T;       // (k t) mod T
    const float ang = __fdiv_rn((float)(2 * q), (float)T);
    const float in = fmaf(z(2 * k), sinpif(ang), __fmul_rn(z(2 * k - 1), cospif(ang)));
    acc = fmaf(cw[k], in, acc);
  }
  if (!(T & 1)) acc = fmaf((t & 1) ? -cw[k] : cw[k], z(T - 1), acc);     // (k == T / 2 here)
  return acc;
}

// 0: row s is a fresh sample (rows past the pool's end, which a partial tile touches, count as fresh: a pure function,
// nothing read), 1: carried row s - Nit of keep, 2: the mean
__device__ __forceinline__ int icem_row_kind(const IcemPool& p, int s) {
  if (s < p.Nit) return 0;
  if (s < p.Nit + p.carry) return 1;
  return s == p.Nit + p.carry && p.addmean ? 2 : 0;
}

// The control j of step t of pool row s of problem b: the only place a pool row's control is formed (the rollout
// and k_icem_update both call it).  mean / sd: the problem's [T][m]; keep: the problem's [nkeep][T][m]; z(k): the k-th
// normal of (s, j), asked for on coloured fresh rows only.  The clamp is cem_control's: two selects.
template <typename Z>
__device__ __forceinline__ float icem_control(const IcemPool& p, const CemRng& g, int b, int s, int t, int j, int T,
                                              int m, const float* mean, const float* sd, const float* keep, float lo,
                                              float hi, Z z) {
  const int kind = icem_row_kind(p, s), e = t * m + j;
  if (kind == 0 && p.white) return cem_control(g, b, s, t, j, m, mean[e], sd[e], lo, hi);
  float u;
  if (kind == 0)
    u = fmaf(sd[e], icem_colour(p.cw, T, t, z), mean[e]);
  else
    u = kind == 1 ? keep[(size_t)(s - p.Nit) * T * m + e] : mean[e];
  u = u < lo ? lo : u;
  u = u > hi ? hi : u;
  return u;
}

// ---- the rollout ----------------------------------------------------------------------------------------------
struct IcemDrawn {
  using Args = IcemRollArgs;
  static __host__ __device__ __forceinline__ const CemRollArgs& roll(const Args& a) { return a.c; }
  static __host__ __device__ __forceinline__ int rows(const Args& a) { return a.p.Nit + a.p.carry + a.p.addmean; }
  static __host__ __device__ __forceinline__ int ldc(const Args& a) { return a.ldc; }
  // The pool's own refusals; zlds where the normals of a tile -- 32 m T floats -- fit behind the operand blocks (the
  // controls are the same either way)
  static int plan(Args& a, size_t blocks, size_t* extra) {
    if (a.p.Nit < 1 || a.p.Nit > a.c.N || a.p.carry < 0 || a.p.carry > a.p.nkeep) return 1;
    if (a.p.carry > 0 && !a.p.keep) return 1;
    if (!a.p.white && !a.p.cw) return 1;
    const size_t z = (size_t)GMPC_CEM_ROWS * a.c.m * a.c.T * sizeof(float);
    a.zlds = !a.p.white && blocks + z <= GMPC_SAMPLED_LDS_BYTES;
    *extra = a.zlds ? z : 0;
    return 0;
  }

  const IcemRollArgs& q;
  float* zl;                  // zlds: [32][m][T] normals of the tile's fresh rows, behind the operand blocks
  const float *mean, *sd, *keep;
  __device__ __forceinline__ IcemDrawn(const Args& a, char* behind)
      : q(a), zl(reinterpret_cast<float*>(behind)), mean(nullptr), sd(nullptr), keep(nullptr) {}
  __device__ __forceinline__ void begin(int b, int s0, int tid) {
    const int T = q.c.T, m = q.c.m;
    mean = q.c.mean + (size_t)b * T * m;
    sd = q.c.sd + (size_t)b * T * m;
    keep = q.p.keep ? q.p.keep + (size_t)b * q.p.nkeep * T * m : nullptr;
    if (!q.zlds) return;
    for (int e = tid; e < GMPC_CEM_ROWS * m * T; e += GMPC_DG_THREADS) {
      const int ij = e / T, k = e - ij * T, i = ij / m, j = ij - i * m;
      zl[e] = icem_row_kind(q.p, s0 + i) == 0 ? cem_normal(q.c.rng, b, s0 + i, k * m + j) : 0.f;
    }
    __syncthreads();
  }
  __device__ __forceinline__ float control(int b, int i, int s, int t, int j) const {
    const int T = q.c.T, m = q.c.m;
    const float lo = q.c.lo ? q.c.lo[j] : -INFINITY, hi = q.c.hi ? q.c.hi[j] : INFINITY;
    if (q.zlds) {
      const float* zr = zl + (i * m + j) * T;
      return icem_control(q.p, q.c.rng, b, s, t, j, T, m, mean, sd, keep, lo, hi, [zr](int k) { return zr[k]; });
    }
    const CemRng& g = q.c.rng;
    return icem_control(q.p, g, b, s, t, j, T, m, mean, sd, keep, lo, hi,
                        [&g, b, s, j, m](int k) { return cem_normal(g, b, s, k * m + j); });
  }
  __device__ __forceinline__ void record(int b, int s, int t, int j, float u) const {
    const int N = q.c.N, T = q.c.T, m = q.c.m;
    if (q.c.samples && s < q.p.Nit) q.c.samples[(((size_t)b * N + s) * T + t) * m + j] = u;
  }
};

template __global__ void k_sampled_rollout<IcemDrawn, false, CemOneModel>(IcemRollArgs, CemOneModel);
template __global__ void k_sampled_rollout<IcemDrawn, true, CemOneModel>(IcemRollArgs, CemOneModel);
template __global__ void k_sampled_rollout<IcemDrawn, false, CemMember>(IcemRollArgs, CemMember);
template __global__ void k_sampled_rollout<IcemDrawn, true, CemMember>(IcemRollArgs, CemMember);
template __global__ void k_sampled_rollout<IcemDrawn, false, CemParticle>(IcemRollArgs, CemParticle);
template __global__ void k_sampled_rollout<IcemDrawn, true, CemParticle>(IcemRollArgs, CemParticle);
template __global__ void k_sampled_rollout<IcemDrawn, false, CemDisagree>(IcemRollArgs, CemDisagree);
template __global__ void k_sampled_rollout<IcemDrawn, true, CemDisagree>(IcemRollArgs, CemDisagree);

// ---- the update -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GMPC_DG_THREADS) void k_icem_update(IcemUpdArgs a, int P) {
  extern __shared__ __attribute__((aligned(16))) char smem_iu[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem_iu);   // [P], P the power of two >= rows
  float* st = reinterpret_cast<float*>(keys + P);                              // [a.stage][T m] staged controls
  const int tid = threadIdx.x, b = blockIdx.x, E = a.E, T = a.T, m = a.m, Tm = T * m;
  const int rows = a.p.Nit + a.p.carry + a.p.addmean, nkeep = a.p.nkeep;
  const float* costs = a.costs + (size_t)b * a.ldc;
  for (int i = tid; i < P; i += GMPC_DG_THREADS) keys[i] = i < rows ? cem_key(costs[i], i) : ~0ull;
  __syncthreads();
  cem_sort_keys(keys, P, tid);
  if (a.elites)
    for (int r = tid; r < E; r += GMPC_DG_THREADS) a.elites[(size_t)b * E + r] = (int)(uint32_t)keys[r];
  // the cheapest row against the best so far (strictly cheaper: never a NaN)
  const float c0 = costs[(int)(uint32_t)keys[0]];
  const bool alive = fabsf(c0) < INFINITY;     // some cost is finite: otherwise mean and std stay, bit for bit
  const float best_old = a.best_cost ? a.best_cost[b] : INFINITY;
  const bool improve = a.best_cost && c0 < best_old;
  const float best_new = improve ? c0 : best_old;
  const bool give_best = a.return_best && a.best_cost && fabsf(best_new) < INFINITY;
  __syncthreads();      // every thread has read best_cost[b]
  if (tid == 0 && improve) a.best_cost[b] = c0;
  const float* mean = a.mean + (size_t)b * Tm;
  const float* sd = a.sd + (size_t)b * Tm;
  const float* keep = a.p.keep ? a.p.keep + (size_t)b * nkeep * Tm : nullptr;
  const CemRng& g = a.rng;
  // the control (t, j) of the elite of rank r, and where it goes beside the sums
  auto elite = [&](int r, int e) {
    const int t = e / m, j = e - t * m, s = (int)(uint32_t)keys[r];
    const float lo = a.lo ? a.lo[j] : -INFINITY, hi = a.hi ? a.hi[j] : INFINITY;
    const float u = icem_control(a.p, g, b, s, t, j, T, m, mean, sd, keep, lo, hi,
                                 [&g, b, s, j, m](int k) { return cem_normal(g, b, s, k * m + j); });
    if (r < nkeep) a.keep_out[((size_t)b * nkeep + r) * Tm + e] = u;
    if (r == 0 && improve) a.best_U[(size_t)b * Tm + e] = u;
    return u;
  };
  const float fE = (float)E, gm = a.gamma, g1 = 1.f - a.gamma;
  // mean / sd / U_out of element e from its sums; u0: the rank-0 control of the element
  auto finish = [&](int e, float sum_nm, float ss, float u0) {
    const size_t o = (size_t)b * Tm + e;
    const float mu = a.mean[o], sg = a.sd[o];
    float nmean = mu;
    if (alive) {
      nmean = __fadd_rn(__fmul_rn(gm, mu), __fmul_rn(g1, sum_nm));
      a.mean[o] = nmean;
      a.sd[o] = __fadd_rn(__fmul_rn(gm, sg), __fmul_rn(g1, sqrtf(ss / fE)));
    }
    if (a.last && a.U_out) a.U_out[o] = give_best ? (improve ? u0 : a.best_U[o]) : nmean;
  };
  if (a.stage > 0) {
    // Fewer elements than threads (T m < 256): one element per thread would leave most of the workgroup idle behind
    // 2 E regenerations each.  Blocks of a.stage elites instead: every thread forms controls into LDS, then thread e
    // adds its column in rank order -- the same terms in the same order as the loop below.
    float sum = 0.f, u0 = 0.f;
    for (int r0 = 0; r0 < E; r0 += a.stage) {
      const int cnt = min(a.stage, E - r0);
      for (int i = tid; i < cnt * Tm; i += GMPC_DG_THREADS) st[i] = elite(r0 + i / Tm, i % Tm);
      __syncthreads();
      if (tid < Tm) {
        if (r0 == 0) u0 = st[tid];
        for (int k = 0; k < cnt; ++k) sum += st[k * Tm + tid];
      }
      if (r0 + cnt < E) __syncthreads();     // (the last block stays in LDS)
    }
    const float nm = sum / fE;
    float ss = 0.f;
    for (int r0 = 0; r0 < E; r0 += a.stage) {
      const int cnt = min(a.stage, E - r0);
      if (E > a.stage) {                     // more than one block: regenerate it (the same values)
        __syncthreads();
        for (int i = tid; i < cnt * Tm; i += GMPC_DG_THREADS) st[i] = elite(r0 + i / Tm, i % Tm);
        __syncthreads();
      }
      if (tid < Tm)
        for (int k = 0; k < cnt; ++k) {
          const float d = st[k * Tm + tid] - nm;
          ss = __fadd_rn(ss, __fmul_rn(d, d));
        }
    }
    __syncthreads();    // every read of a.mean / a.sd by elite() has been made
    if (tid < Tm) finish(tid, nm, ss, u0);
    return;
  }
  // one (step, control) per thread: sums over the elites in rank order.  (Element e reads a.mean / a.sd at e only,
  // and writes them behind its last read.)
  for (int e = tid; e < Tm; e += GMPC_DG_THREADS) {
    float sum = 0.f, u0 = 0.f;
    for (int r = 0; r < E; ++r) {
      const float u = elite(r, e);
      if (r == 0) u0 = u;
      sum += u;
    }
    const float nm = sum / fE;
    float ss = 0.f;
    for (int r = 0; r < E; ++r) {
      const float d = elite(r, e) - nm;
      ss = __fadd_rn(ss, __fmul_rn(d, d));
    }
    finish(e, nm, ss, u0);
  }
}

// Host-side launchers ---------------------------------------------------------------------------
int gmpc_launch_sampled_rollout(const IcemRollArgs& a, bool bf16, const CemEnsemble* ens, hipStream_t s) {
  return sampled_launch_rollout<IcemDrawn>(a, bf16, ens, s);
}

int gmpc_launch_icem_update(const IcemUpdArgs& a0, hipStream_t s) {
  IcemUpdArgs a = a0;
  const int rows = a.p.Nit + a.p.carry + a.p.addmean, Tm = a.T * a.m;
  if (a.p.Nit < 1 || rows > GMPC_CEM_MAX_N || a.ldc < rows || a.E < 1 || a.E > rows || a.p.nkeep > a.E) return 1;
  if (a.p.nkeep > 0 && !a.keep_out) return 1;
  if ((a.best_cost != nullptr) != (a.best_U != nullptr)) return 1;
  int P = 1;
  while (P < rows) P <<= 1;
  a.stage = Tm < GMPC_DG_THREADS ? GMPC_ICEM_STAGE_FLOATS / Tm : 0;
  const size_t lds = (size_t)P * sizeof(unsigned long long) + (a.stage ? GMPC_ICEM_STAGE_FLOATS * sizeof(float) : 0);
  hipLaunchKernelGGL(k_icem_update, dim3(a.B), dim3(GMPC_DG_THREADS), lds, s, a, P);
  return 0;
}
