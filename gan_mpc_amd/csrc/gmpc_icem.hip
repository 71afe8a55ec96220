// The sample-efficient cross-entropy method (gmpc_icem_solve; Pinneri et al., CoRL 2020) on the
// sampled rollout of the cross-entropy method.  Per iteration a pool of rows per problem -- fresh samples with
// power-law ("coloured") noise along the horizon, the rows kept from the iteration before, in the last iteration the
// mean itself -- is rolled out and costed (k_icem_rollout: the body of k_cem_rollout over another source of
// controls); the E cheapest by (cost, row) refit mean and std, the cheapest of them become the next kept rows, and
// the best row seen so far is remembered (k_icem_update).  As in gmpc_cem.hip no noise and no sample is stored: a
// fresh control is a pure function of (seed, iteration, problem, sample, step, control) -- icem_control, the one
// place a pool row's control is formed -- and the update regenerates the elites' controls.
//
//   k_icem_rollout  one 256-thread workgroup per 32 pool rows of one problem (cem_rollout_body).  The coloured sum of
//                   a control needs the T normals of its (row, control): formed once per tile in LDS behind the
//                   operand block where 32 m T floats fit there (zlds), regenerated per element otherwise -- the
//                   same sum in the same order either way.
//   k_icem_rollout_ens, k_icem_rollout_ens_bf16  the pool's rows under every member of a dynamics ensemble (DESIGN.md
//                   section 24; blockIdx.y: the member), followed by k_ens_reduce of gmpc_cem.hip
//   k_icem_update   one workgroup per problem: the sort of k_cem_update over the pool's rows, then the elites' sums in
//                   rank order (for T m < 256 by the whole workgroup, in blocks of elites staged in LDS: the same
//                   sums), the kept rows, the best row and the returned sequence.
#include "gmpc_cem_rollout.h"

#include <cstring>

#define GMPC_ICEM_STAGE_FLOATS 4096   // k_icem_update's staged controls (16 KiB of LDS behind the keys)
#define GMPC_ICEM_LDS_BYTES 65536     // dynamic LDS a launch may ask for without opting in to more

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

// The control j of step t of pool row s of problem b: the only place a pool row's control is formed (k_icem_rollout
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
  const IcemRollArgs& q;
  float* zl;                  // zlds: [32][m][T] normals of the tile's fresh rows, behind the operand block
  const float *mean, *sd, *keep;
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

__global__ __launch_bounds__(GMPC_DG_THREADS) void k_icem_rollout(IcemRollArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_icem[];
  float* Ab = reinterpret_cast<float*>(smem_icem);  // [32][GMPC_DG_LDA]: the layer inputs of the 32 pool rows
  IcemDrawn src{a, Ab + GMPC_CEM_ROWS * GMPC_DG_LDA, nullptr, nullptr, nullptr};
  cem_rollout_body<false>(a.c, a.p.Nit + a.p.carry + a.p.addmean, a.ldc, Ab, nullptr, src);
}

// The same rows with bf16 matrix operands: a.c.dyn.W / a.c.cost.W are the packed bf16 images,
// and the normals of zlds lie behind both operand blocks
__global__ __launch_bounds__(GMPC_DG_THREADS) void k_icem_rollout_bf16(IcemRollArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_icem16[];
  float* Ab = reinterpret_cast<float*>(smem_icem16);
  __bf16* Hb = reinterpret_cast<__bf16*>(Ab + GMPC_CEM_ROWS * GMPC_DG_LDA);
  IcemDrawn src{a, reinterpret_cast<float*>(smem_icem16 + GMPC_CEM_LDS16), nullptr, nullptr, nullptr};
  cem_rollout_body<true>(a.c, a.p.Nit + a.p.carry + a.p.addmean, a.ldc, Ab, Hb, src);
}

// The same pool rows under every member of a dynamics ensemble (blockIdx.y: the member)
__global__ __launch_bounds__(GMPC_DG_THREADS) void k_icem_rollout_ens(IcemRollArgs a, CemMember e) {
  extern __shared__ __attribute__((aligned(16))) char smem_icem_e[];
  float* Ab = reinterpret_cast<float*>(smem_icem_e);
  IcemDrawn src{a, Ab + GMPC_CEM_ROWS * GMPC_DG_LDA, nullptr, nullptr, nullptr};
  cem_rollout_body<false>(a.c, a.p.Nit + a.p.carry + a.p.addmean, a.ldc, Ab, nullptr, src, e);
}

__global__ __launch_bounds__(GMPC_DG_THREADS) void k_icem_rollout_ens_bf16(IcemRollArgs a, CemMember e) {
  extern __shared__ __attribute__((aligned(16))) char smem_icem_e16[];
  float* Ab = reinterpret_cast<float*>(smem_icem_e16);
  __bf16* Hb = reinterpret_cast<__bf16*>(Ab + GMPC_CEM_ROWS * GMPC_DG_LDA);
  IcemDrawn src{a, reinterpret_cast<float*>(smem_icem_e16 + GMPC_CEM_LDS16), nullptr, nullptr, nullptr};
  cem_rollout_body<true>(a.c, a.p.Nit + a.p.carry + a.p.addmean, a.ldc, Ab, Hb, src, e);
}

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
// ens: null, or the ensemble whose members all roll the pool out (a.c.dyn: member 0), followed by the reduce
static int icem_launch_rollout(const IcemRollArgs& a, bool bf16, hipStream_t s, const CemEnsemble* ens = nullptr) {
  const CemRollArgs& c = a.c;
  if (ens && (ens->P < 1 || ens->P > GMPC_MAX_ENSEMBLE || !ens->part || c.X || c.mean_row)) return 1;
  for (int l = 0; l <= c.dyn.L; ++l)
    if (c.dyn.dims[l] > 256) return 1;
  for (int l = 0; l <= c.cost.L; ++l)
    if (c.cost.dims[l] > 256) return 1;
  const int rows = a.p.Nit + a.p.carry + a.p.addmean;
  if (c.n + c.m > 256 || a.p.Nit < 1 || a.p.carry < 0 || a.p.carry > a.p.nkeep || rows > GMPC_CEM_MAX_N ||
      a.ldc < rows || a.p.Nit > c.N)
    return 1;
  if (a.p.carry > 0 && !a.p.keep) return 1;
  if (!a.p.white && !a.p.cw) return 1;
  size_t lds = bf16 ? GMPC_CEM_LDS16 : GMPC_CEM_LDS32;
  if (a.zlds) lds += (size_t)GMPC_CEM_ROWS * c.m * c.T * sizeof(float);
  if (lds > GMPC_ICEM_LDS_BYTES) return 1;
  const int tiles = (rows + GMPC_CEM_ROWS - 1) / GMPC_CEM_ROWS;
  if (ens) {
    const CemMember mb{ens->wstride, ens->bstride, (size_t)c.B * a.ldc, ens->part};
    if (bf16)
      hipLaunchKernelGGL(k_icem_rollout_ens_bf16, dim3(c.B * tiles, ens->P), dim3(GMPC_DG_THREADS), lds, s, a, mb);
    else
      hipLaunchKernelGGL(k_icem_rollout_ens, dim3(c.B * tiles, ens->P), dim3(GMPC_DG_THREADS), lds, s, a, mb);
    gmpc_launch_ens_reduce(*ens, c.B, rows, a.ldc, c.costs, s);
    return 0;
  }
  if (bf16)
    hipLaunchKernelGGL(k_icem_rollout_bf16, dim3(c.B * tiles), dim3(GMPC_DG_THREADS), lds, s, a);
  else
    hipLaunchKernelGGL(k_icem_rollout, dim3(c.B * tiles), dim3(GMPC_DG_THREADS), lds, s, a);
  return 0;
}

int gmpc_launch_icem_rollout(const IcemRollArgs& a, hipStream_t s) { return icem_launch_rollout(a, false, s); }
int gmpc_launch_icem_rollout_bf16(const IcemRollArgs& a, hipStream_t s) { return icem_launch_rollout(a, true, s); }
int gmpc_launch_icem_rollout_ens(const IcemRollArgs& a, const CemEnsemble& e, bool bf16, hipStream_t s) {
  return icem_launch_rollout(a, bf16, s, &e);
}

// The shapes whose normals k_icem_rollout forms once per tile in LDS: 32 m T floats beside the operand block (bf16:
// beside both blocks of k_icem_rollout_bf16; the controls are the same either way)
int gmpc_icem_zlds(int T, int m, int bf16) {
  return (size_t)(bf16 ? GMPC_CEM_LDS16 : GMPC_CEM_LDS32) + (size_t)GMPC_CEM_ROWS * m * T * sizeof(float) <=
         GMPC_ICEM_LDS_BYTES;
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
