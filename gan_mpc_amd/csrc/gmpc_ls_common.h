// What the kernels that evaluate line-search candidates share (k_traj<true>, k_traj_rw<true>, k_ls16, k_ls32) and, on
// the host, what the launchers of k_ls16 / k_ls32 share.  The round protocol itself -- work list, decide, commit, and
// the plan that says which of these kernels takes part -- is gmpc_linesearch.hip.
#pragma once
#include "gmpc_device.h"

// ---- which kernel evaluates a round --------------------------------------------------------------------------------
// A round's launches all read the round's candidate count and all but one return at once: the owner of a count is
// decided here and nowhere else.  The plan (gmpc_ls_plan) guarantees 1 <= ls_split <= ls32_split for the thresholds
// that are in use (0: that form does not take part), so the three ranges partition the counts.
enum LsForm { LS_FORM_RW = 0, LS_FORM_16, LS_FORM_32 };
__device__ __forceinline__ LsForm ls_round_form(int cnt, const TrajArgs& a) {
  if (a.ls32_split > 0 && cnt >= a.ls32_split) return LS_FORM_32;   // more than one pass of k_ls16 over the chip
  if (a.ls_split > 0 && cnt >= a.ls_split) return LS_FORM_16;       // long work list
  return LS_FORM_RW;                                                // short work list: 4 candidates per workgroup
}

// ---- a workgroup's candidate table ---------------------------------------------------------------------------------
// step size of halving count k (trajax line_search_ddp halves alpha_0 k times, it does not scale by 2^-k)
__device__ __forceinline__ float ls_alpha(float alpha_0, int k) {
  float al = alpha_0;
  for (; k > 0; --k) al *= 0.5f;
  return al;
}
// item `item` of the round's work list of `cnt` items: its trajectory, whether it exists (a workgroup's slots past the
// end of the list read the last item and write nothing) and its step size
__device__ __forceinline__ void ls_candidate(const TrajArgs& a, int cnt, int item, int* bi, int* in, float* alpha) {
  const int it = min(item, cnt - 1);
  *bi = a.item_b[it];
  *in = item < cnt;
  *alpha = ls_alpha(a.alpha_0, a.item_k[it]);
}

// ---- cycle stamps of the GMPC_TRAJ_STAMPS diagnostic build -----------------------------------------------------------
// TS_BEGIN() starts the accumulator, TS_(i) adds the cycles since the previous stamp to st_[i]; each kernel prints its
// own st_ after the horizon
#ifdef GMPC_TRAJ_STAMPS
#define TS_BEGIN() unsigned long long st_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tp_ = __builtin_readcyclecounter()
#define TS_(i) { const unsigned long long t_ = __builtin_readcyclecounter(); st_[i] += t_ - tp_; tp_ = t_; }
#else
#define TS_BEGIN()
#define TS_(i)
#endif

// ---- 16 candidates on v_mfma_f32_16x16x4_f32 (k_ls16, and each of k_ls32's two groups) ----------------------------
#define LS_C 16            // candidates per group: the 16-column operand
#define LS_KH 200          // hidden width of the form with the K-split row block 12
#define LS_KS 50           // its k-steps per hidden layer
#define LS_GS 80           // floats between groups of 4 activation rows
#define LS_ROWS 208        // activation rows (13 blocks)

__device__ __forceinline__ f32x4_t ls_mfma(float a, float b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// float index of activation row k, candidate c
__device__ __forceinline__ int ls_at(int k, int c) { return (k >> 2) * LS_GS + (k & 3) * 16 + c; }

// bias table [3][208] hidden biases (rows >= kh: 0), [32] output bias (rows >= n: 0), filled by `nthreads` threads
__device__ __forceinline__ void ls_fill_bias(float* bias_s, const MlpDesc& dyn, int kh, int n, int tid, int nthreads) {
  for (int e = tid; e < 3 * LS_ROWS + 32; e += nthreads) {
    float v = 0.f;
    if (e < 3 * LS_ROWS) {
      const int l = e / LS_ROWS, j = e - l * LS_ROWS;
      if (j < kh) v = dyn.b[l][j];
    } else if (e - 3 * LS_ROWS < n) {
      v = dyn.b[3][e - 3 * LS_ROWS];
    }
    bias_s[e] = v;
  }
}

// The three functions below run after the horizon on the 256 threads of one group (tt: thread of the group; wave,
// lane: its wave of the group and its lane, handed in as the kernels hold them -- with the lane derived again in here
// hipcc allocates and schedules k_ls32's time loop differently, and that loop is tuned).  BI(c) / INB(c) / CI(c):
// trajectory, existence and candidate index of the group's candidate c.  k_ls16 and k_ls32 must agree bit for bit
// (tests: test_linesearch_two_group_form_is_bit_identical): this is the one copy both run.

// stage costs cst[16][T]: 4 lanes per (candidate, step) pair, 64 pairs per sweep
template <class FBI, class FINB, class FCI>
__device__ __forceinline__ void ls_stage_costs(const TrajArgs& a, int tt, float w0, float w1, float* cst, FBI BI,
                                               FINB INB, FCI CI) {
  const int n = a.n, m = a.m, T = a.T;
  const float al = GMPC_ALPHA;
  const int q = tt & 3;
  for (int p = tt >> 2; p < LS_C * T; p += 64) {
    const int c = p / T, t = p - c * T;
    const int bc = BI(c);
    const size_t ci = INB(c) ? (size_t)CI(c) : 0;          // (unused candidates read item 0's rows: in bounds, discarded)
    const float* xr = t > 0 ? a.Xc + (ci * (T + 1) + t) * n : a.X + (size_t)bc * (T + 1) * n;
    const float* ur = a.Uc + (ci * T + t) * m;
    const float* gl = a.goal + ((size_t)bc * (T + 1) + t) * n;
    float xv[8], gv[8], uv[2];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int i = min(q + 4 * e, n - 1);
      xv[e] = xr[i];
      gv[e] = gl[i];
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) uv[e] = ur[min(q + 4 * e, m - 1)];
    float dd = 0.f, uu = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float dx = q + 4 * e < n ? xv[e] - gv[e] : 0.f;
      dd = fmaf(dx, dx, dd);
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const float u = q + 4 * e < m ? uv[e] : 0.f;
      uu = fmaf(u, u, uu);
    }
    dd += __shfl_xor(dd, 1); dd += __shfl_xor(dd, 2);
    uu += __shfl_xor(uu, 1); uu += __shfl_xor(uu, 2);
    if (q == 0) cst[p] = INB(c) ? w0 * (sqrtf(uu + al * al) - al) + w1 * (sqrtf(dd + al * al) - al) : 0.f;
  }
}
// a candidate's stage costs summed in step order (the sum trajax' evaluate builds)
__device__ __forceinline__ float ls_cost_sum(const float* cst, int T) {
  float acc = 0.f;
  for (int t = 0; t < T; ++t) acc += cst[t];
  return acc;
}
// terminal cost w2 |cost_mlp(x_T)|^2 on the matrix pipe as well, and the candidates' objectives sobj[c] + terminal
// -> objc: activations [k][16] in actA / actB, weight fragments straight from global memory (row blocks nb = wave,
// wave + 4, ..).  Workgroup barriers inside: every thread of the workgroup calls it.
template <class FINB, class FCI>
__device__ __forceinline__ void ls_terminal_cost(const TrajArgs& a, int tt, int wave, int lane, float w2, const float* xcur,
                                                 float* actA, float* actB, const float* sobj, FINB INB, FCI CI) {
  const int n = a.n, g = lane >> 4, c16 = lane & 15;
  float* in = actA;
  float* out = actB;
  for (int e = tt; e < LS_C * ((n + 3) & ~3); e += 256) {
    const int i = e >> 4, c = e & 15;
    in[ls_at(i, c)] = i < n ? xcur[ls_at(i, c)] : 0.f;
  }
  __syncthreads();
  const int Lc = a.cost.L - 1;
  for (int l = 0; l <= Lc; ++l) {
    const int fi = a.cost.dims[l], fo = a.cost.dims[l + 1];
    const float* W = a.cost.W[l];
    const float* bv = a.cost.b[l];
    const int nks = (fi + 3) >> 2;
    for (int nb = wave; 16 * nb < fo; nb += 4) {
      const int col = 16 * nb + c16;
      const bool colok = col < fo;
      f32x4_t acc;
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = 16 * nb + 4 * g + i < fo ? bv[16 * nb + 4 * g + i] : 0.f;
      const float* wp = W + (colok ? col : 0);
      for (int k0 = 0; k0 < nks; k0 += 8) {        // 8 fragments in flight (k-steps past the last: zero weights)
        float wv[8], bq[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int ks = min(k0 + e, nks - 1), k = 4 * ks + g;
          const float w = wp[(size_t)min(k, fi - 1) * fo];
          wv[e] = (k0 + e < nks && k < fi && colok) ? w : 0.f;
          bq[e] = in[ks * LS_GS + lane];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = ls_mfma(wv[e], bq[e], acc);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float v = l < Lc ? fmaxf(acc[i], 0.f) : acc[i];
        if (16 * nb + 4 * g + i >= fo) v = 0.f;
        out[(4 * nb + g) * LS_GS + i * 16 + c16] = v;
      }
    }
    __syncthreads();
    float* tmp = in; in = out; out = tmp;
  }
  if (tt < LS_C && INB(tt)) {
    const int fo = a.cost.dims[Lc + 1];
    float yy = 0.f;
    for (int r = 0; r < fo; ++r) {
      const float y = in[ls_at(r, tt)];
      yy = fmaf(y, y, yy);
    }
    a.objc[CI(tt)] = sobj[tt] + w2 * yy;
  }
}

// ---- host side: what the launchers of k_ls16 / k_ls32 share ---------------------------------------------------------
// The <K0S, NOB> instantiation for (n, m) -- K0S: k-steps of layer 0 (n + m <= 4 K0S), NOB: 16-row blocks of the output
// layer (n <= 16 NOB) --, handed to f as two integral constants
template <class F>
static void ls_pick_k0s_nob(int n, int m, F f) {
  using std::integral_constant;
  if (n > 16) f(integral_constant<int, 6>{}, integral_constant<int, 2>{});
  else if ((n + m + 3) / 4 <= 4) f(integral_constant<int, 4>{}, integral_constant<int, 1>{});
  else f(integral_constant<int, 6>{}, integral_constant<int, 1>{});
}
// launch of kernel Kern with TrajArgs; dynamic LDS above the default 64 KB needs the attribute, set once per kernel
template <auto Kern>
static void ls_launch(int lds_max, int grid, int threads, size_t lds, hipStream_t s, const TrajArgs& a) {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
    (void)hipGetLastError();
    attr = true;
  }
  hipLaunchKernelGGL(Kern, dim3(grid), dim3(threads), lds, s, a);
}
