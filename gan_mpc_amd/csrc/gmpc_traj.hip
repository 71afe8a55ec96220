// Sequential-in-time trajectory kernels: rollout + cost, and the candidates of the DDP line search.  This file holds
// the general (any network shape) VALU form, the mask-only forward pass and their launchers; the reference's default
// dynamics network (3 x 200) takes the register-weight MFMA form of gmpc_traj_rw.hip, and the line search's rounds
// (work list, decide, commit, and which kernel evaluates a round) are gmpc_linesearch.hip.
//
// One 256-thread workgroup owns GMPC_TB = 4 trajectories for the whole horizon.  The state and
// control of the current step live in LDS as float4 (one component per trajectory), every layer is
// "one output neuron per thread": the weight row is read coalesced from L2 once and reused for
// the four trajectories from registers.  relu sign bits leave the kernel as ballot bitmasks so the
// backward Jacobian chain never recomputes the forward pass.
//
// Reference arithmetic: dynamics/nn.py:27-34 (residual relu MLP), cost/cost_model.py:20-42,
// cost/nn.py:23-29, trajax rollout / evaluate / ddp_rollout / line_search_ddp as called from
// policy/optimizers.py:19,26-29,55.
#include "gmpc_traj_layers.h"
#include "gmpc_ls_common.h"
#include "gmpc_launch.h"

#ifndef GMPC_TRAJ_MINW
#define GMPC_TRAJ_MINW 4
#endif
#define GMPC_TRAJ_THREADS 512   // k_traj: 8 waves, the upper 4 take the second half of every K range

template <bool LS>
__global__ __launch_bounds__(GMPC_TRAJ_THREADS, GMPC_TRAJ_MINW) void k_traj(TrajArgs a) {
  // dynamic LDS: actA | actB (aw float4 each: max(n+m, widest layer)) | part (pw) | ksp (256) | xcur (n)
  extern __shared__ __attribute__((aligned(16))) char smem_traj[];
  float4* const actA = reinterpret_cast<float4*>(smem_traj);
  float4* const actB = actA + a.aw;
  float4* const part = actB + a.aw;
  float4* const ksp = part + a.pw;
  float4* const xcur = ksp + GMPC_THREADS;
  // the two small weight matrices live in LDS for the whole horizon when they fit (launcher decides)
  float* const w0_s = reinterpret_cast<float*>(xcur + a.n);
  float* const wl_s = w0_s + a.sw0;
  __shared__ float s_alpha[GMPC_TB], s_oo[GMPC_TB];
  __shared__ int s_bi[GMPC_TB], s_in[GMPC_TB], s_live[GMPC_TB];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n = a.n, m = a.m, T = a.T;
  // slot c of this block: plain rollout -> trajectory b0 + c; line search -> item b0 + c of the
  // round's work list, i.e. one (trajectory, step size) candidate
  const int b0 = blockIdx.x * GMPC_TB;
  if (LS) {
    const int cnt = *a.nitems;
    if (b0 >= cnt) return;
    if (tid < GMPC_TB) {
      ls_candidate(a, cnt, b0 + tid, &s_bi[tid], &s_in[tid], &s_alpha[tid]);
      // the objective to beat: stage and terminal costs are non-negative, so a candidate whose
      // running sum has reached it can no longer be accepted (NaN compares false: dead as well)
      float oo = a.obj[s_bi[tid]];
      if (isnan(oo)) oo = INFINITY;
      s_oo[tid] = oo;
      s_live[tid] = s_in[tid];
    }
  } else if (tid < GMPC_TB) {
    s_bi[tid] = min(b0 + tid, a.B - 1);
    s_in[tid] = (b0 + tid) < a.B;
  }
  __syncthreads();
  // Component c of an LDS float4 is always addressed as a float ([k*4 + c]) when c is a run-time
  // value: one address computation instead of the branch tree hipcc builds for `c == 0 ? v.x : ...` on an
  // LDS reference.  (Round 1 saw that tree hand lanes with c == 3 the .z address inside this kernel; the
  // pattern in isolation compiles and runs correctly, tests/repro/README.md.)
  float* const xf = reinterpret_cast<float*>(xcur);
  float* const aAf = reinterpret_cast<float*>(actA);
  const float* const pf = reinterpret_cast<const float*>(part);
  // trajectory c of this block (reads of the tail block are clamped); no private arrays: a
  // dynamically indexed register array would live in scratch
  auto BI = [&](int c) -> int { return s_bi[c]; };
  auto INB = [&](int c) -> bool { return s_in[c] != 0; };
  // candidate (item) index of slot c: where the line search writes X / U / masks / objective
  auto CI = [&](int c) -> size_t { return (size_t)(b0 + c); };
  const int Lh = a.dyn.L - 1;
  const size_t mstride = (size_t)T * Lh * GMPC_MW;   // mask words per trajectory
  for (int e = tid; e < a.sw0; e += blockDim.x) w0_s[e] = a.dyn.W[0][e];
  for (int e = tid; e < a.swl; e += blockDim.x) wl_s[e] = a.dyn.W[Lh][e];
  const float* const W0 = a.sw0 ? w0_s : a.dyn.W[0];
  const float* const WL = a.swl ? wl_s : a.dyn.W[Lh];
  const float w0 = sigmoidf_(a.mpc_w[0]), w1 = sigmoidf_(a.mpc_w[1]), w2 = sigmoidf_(a.mpc_w[2]);

  {
    // bit c set: slot c writes its outputs
    unsigned wbits = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) wbits |= (INB(c) ? 1u : 0u) << c;
    // ---- initial state
    for (int i = tid; i < n; i += blockDim.x) {
      const float* xs = LS ? a.X : a.x0;
      const size_t st = LS ? (size_t)(T + 1) * n : (size_t)n;
      float4 v = make_float4(xs[BI(0) * st + i], xs[BI(1) * st + i], xs[BI(2) * st + i],
                             xs[BI(3) * st + i]);
      xcur[i] = v;
      if (!LS) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (INB(c)) a.X[(size_t)BI(c) * (T + 1) * n + i] = f4get(v, c);
      }
    }
    float objacc = 0.f;  // lane 0 of wave c accumulates trajectory c
    // goal of the NEXT step, one element per lane of wave c (n <= 64): its load overlaps a whole step
    float gnext = 0.f;
    if (n <= 64 && wave < GMPC_TB && lane < n) gnext = a.goal[(size_t)BI(wave) * (T + 1) * n + lane];
    __syncthreads();
    TS_BEGIN();

    bool aborted = false;
    for (int t = 0; t < T; ++t) {
      // line search: stop as soon as none of the four candidates can still be accepted (flags of the
      // previous step's cost evaluation; the barriers of that step ordered them)
      if (LS && t > 0 && (s_live[0] | s_live[1] | s_live[2] | s_live[3]) == 0) { aborted = true; break; }
      // ---- controls and layer-0 input
      for (int i = tid; i < n; i += blockDim.x) actA[i] = xcur[i];
      if (LS) {
        // u = U + alpha k + K (x - X_nominal): 16 lanes share one (slot, control) inner product, so
        // the n gain / state loads of a control are issued together instead of one after another
        const int l16 = tid & 15;
        for (int p = tid >> 4; p < GMPC_TB * m; p += GMPC_TRAJ_THREADS >> 4) {
          const int c = p / m, j = p - c * m;
          const int bc = BI(c);
          const size_t ub = ((size_t)bc * T + t) * m + j;
          const float* Kr = a.Kg + ub * n;
          const float* Xo = a.X + ((size_t)bc * (T + 1) + t) * n;
          float du = 0.f;
          for (int i = l16; i < n; i += 16) du = fmaf(Kr[i], xf[i * 4 + c] - Xo[i], du);
          du += __shfl_xor(du, 8);
          du += __shfl_xor(du, 4);
          du += __shfl_xor(du, 2);
          du += __shfl_xor(du, 1);
          if (l16 == 0) {
            const float u = a.Uio[ub] + fmaf(s_alpha[c], a.kg[ub], du);
            if ((wbits >> c) & 1u) a.Uc[(CI(c) * T + t) * m + j] = u;
            aAf[(n + j) * 4 + c] = u;
          }
        }
      } else if (tid < GMPC_TB * m) {
        const int c = tid / m, j = tid % m;
        aAf[(n + j) * 4 + c] = a.U[((size_t)BI(c) * T + t) * m + j];
      }
      __syncthreads();
      TS_(0)
      // ---- stage cost of (x_t, u_t): wave c (< 4) handles trajectory c
      if (wave < GMPC_TB) {
        const int c = wave;
        float dd = 0.f, uu = 0.f;
        const int bc = BI(c);
        const float* g = a.goal + ((size_t)bc * (T + 1) + t) * n;
        if (n <= 64) {
          const float gi = gnext;
          if (lane < n) {
            gnext = g[n + lane];           // row t + 1 (exists: the goal has T + 1 rows)
            const float d = aAf[lane * 4 + c] - gi;
            dd = d * d;
          }
        } else {
          for (int i = lane; i < n; i += 64) {
            const float d = aAf[i * 4 + c] - g[i];
            dd = fmaf(d, d, dd);
          }
        }
        for (int j = lane; j < m; j += 64) {
          const float u = aAf[(n + j) * 4 + c];
          uu = fmaf(u, u, uu);
        }
        dd = wave_sum(dd);
        uu = wave_sum(uu);
        const float al = GMPC_ALPHA;
        const float cst = w0 * (sqrtf(uu + al * al) - al) + w1 * (sqrtf(dd + al * al) - al);
        objacc += cst;
        if (LS && lane == 0) s_live[c] = (INB(c) && objacc < s_oo[c]) ? 1 : 0;
        if (!LS && lane == 0 && INB(c) && a.costs) a.costs[(size_t)bc * (T + 1) + t] = cst;
      }
      TS_(1)
      // ---- hidden layers
      float4* in = actA;
      float4* out = actB;
      for (int l = 0; l < Lh; ++l) {
        // the tail block's clamped trajectories never write (wbits), so b0-relative addressing is safe
        uint32_t* mbase = (LS ? a.maskc : a.masks) + (size_t)b0 * mstride + ((size_t)t * Lh + l) * GMPC_MW;
        hidden_layer(l == 0 ? W0 : a.dyn.W[l], a.dyn.b[l], a.dyn.dims[l], a.dyn.dims[l + 1], in, out, mbase,
                     mstride, wbits, ksp);
        __syncthreads();
        TS_(2 + l)
        float4* tmp = in; in = out; out = tmp;
      }
      // ---- output layer + residual
      if (n <= 32) {
        out_layer32(WL, a.dyn.dims[Lh], n, in, part);
      } else if (n <= (int)blockDim.x) {
        dense_small<1>(WL, a.dyn.dims[Lh], n, in, part);
      } else {
        // wide state (n > 512): one output per thread, chunk after chunk
        for (int jb = 0; jb < n; jb += blockDim.x) {
          float4 acc[1] = {make_float4(0.f, 0.f, 0.f, 0.f)};
          dense_rows<1>(WL, a.dyn.dims[Lh], n, jb + tid, in, acc);
          if (jb + tid < n) part[jb + tid] = acc[0];
        }
        __syncthreads();
      }
      for (int i = tid; i < n; i += blockDim.x) {
        const float bj = a.dyn.b[Lh][i];
        float4 v = part[i];
        const float4 xo = xcur[i];
        v.x = (v.x + bj) + xo.x; v.y = (v.y + bj) + xo.y;
        v.z = (v.z + bj) + xo.z; v.w = (v.w + bj) + xo.w;
        xcur[i] = v;
        float* Xo = LS ? a.Xc : a.X;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if ((wbits >> c) & 1u)
            Xo[((LS ? CI(c) : (size_t)BI(c)) * (T + 1) + t + 1) * n + i] = f4get(v, c);
      }
      __syncthreads();
      TS_(6)
    }
#ifdef GMPC_TRAJ_STAMPS
    if (blockIdx.x == 0 && (tid == 0 || tid == 256))
      printf("tid %d: staging %llu cost %llu L0 %llu L1 %llu L2 %llu out %llu (cycles per step)\n", tid,
             st_[0] / T, st_[1] / T, st_[2] / T, st_[3] / T, st_[4] / T, st_[6] / T);
#endif
    if (LS && aborted) {
      if (tid < GMPC_TB && INB(tid)) a.objc[CI(tid)] = INFINITY;     // rejected without a full rollout
      return;
    }
    // ---- terminal cost w2 * |cost_mlp(x_T)|^2
    {
      float4* in = xcur;
      float4* out = actA;
      const int Lc = a.cost.L - 1;
      for (int l = 0; l < Lc; ++l) {
        hidden_layer(a.cost.W[l], a.cost.b[l], a.cost.dims[l], a.cost.dims[l + 1], in, out, nullptr, 0,
                     0u, ksp);
        __syncthreads();
        in = out;
        out = (out == actA) ? actB : actA;
      }
      const int fo = a.cost.dims[Lc + 1];
      dense_small<1>(a.cost.W[Lc], a.cost.dims[Lc], fo, in, part);
      const int c = wave & (GMPC_TB - 1);
      float yy = 0.f;
      for (int r = lane; r < fo; r += 64) {
        const float y = pf[r * 4 + c] + a.cost.b[Lc][r];
        yy = fmaf(y, y, yy);
      }
      yy = wave_sum(yy);
      const float cst = w2 * yy;
      objacc += cst;
      if (lane == 0 && wave < GMPC_TB) {
        if (!LS) {
          if (INB(c)) {
            if (a.costs) a.costs[(size_t)BI(c) * (T + 1) + T] = cst;
            a.obj[BI(c)] = objacc;
          }
        } else if (INB(c)) {
          a.objc[CI(c)] = objacc;
        }
      }
    }
  }
}

// Forward pass at given (x, u) pairs, masks only: used when gmpc_lqr_backward is handed a
// trajectory that did not come from this context's rollout.  4 samples per workgroup.
__global__ __launch_bounds__(GMPC_THREADS) void k_masks(int NS, int n, int m, int T, MlpDesc dyn,
                                                        const float* X, const float* U,
                                                        uint32_t* masks, int aw) {
  extern __shared__ __attribute__((aligned(16))) char smem_masks[];
  float4* const actA = reinterpret_cast<float4*>(smem_masks);
  float4* const actB = actA + aw;
  const int tid = threadIdx.x;
  const int s0 = blockIdx.x * 4;
  unsigned wbits = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) wbits |= ((s0 + c < NS) ? 1u : 0u) << c;
  for (int i = tid; i < n + m; i += blockDim.x) {
    float4 v;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int si = (s0 + c < NS) ? s0 + c : NS - 1;
      const int b = si / T, t = si % T;
      const float x = i < n ? X[((size_t)b * (T + 1) + t) * n + i]
                            : U[((size_t)b * T + t) * m + (i - n)];
      f4set(v, c, x);
    }
    actA[i] = v;
  }
  __syncthreads();
  const int Lh = dyn.L - 1;
  float4* in = actA;
  float4* out = actB;
  for (int l = 0; l < Lh; ++l) {
    hidden_layer(dyn.W[l], dyn.b[l], dyn.dims[l], dyn.dims[l + 1], in, out,
                 masks + ((size_t)s0 * Lh + l) * GMPC_MW, (size_t)Lh * GMPC_MW, wbits);
    __syncthreads();
    float4* tmp = in; in = out; out = tmp;
  }
}

// Host-side launchers ---------------------------------------------------------------------------
// (traj_aw, the activation width both forms size their LDS with: gmpc_traj_layers.h)
static size_t traj_lds(TrajArgs& a) {
  a.aw = traj_aw(a.n, a.m, a.dyn, &a.cost);
  a.pw = a.n > GMPC_TRAJ_THREADS ? a.n : GMPC_TRAJ_THREADS;
  size_t bytes = ((size_t)2 * a.aw + a.pw + GMPC_THREADS + a.n) * sizeof(float4);
  // W_0 and W_L in LDS while the workgroup stays under 64 KB (two workgroups per CU in the line search)
  const int Lh = a.dyn.L - 1;
  const size_t w0 = (size_t)a.dyn.dims[0] * a.dyn.dims[1], wl = (size_t)a.dyn.dims[Lh] * a.n;
  a.sw0 = a.swl = 0;
  if (bytes + w0 * sizeof(float) <= 64 * 1024) { a.sw0 = (int)w0; bytes += w0 * sizeof(float); }
  if (bytes + wl * sizeof(float) <= 64 * 1024) { a.swl = (int)wl; bytes += wl * sizeof(float); }
  return bytes;
}

// the general form: one workgroup per 4 trajectories (ls = false) / work-list items (ls = true: `grid` covers the
// largest possible work list, the kernel reads the actual count); sizes its own LDS
void gmpc_launch_traj(const TrajArgs& a0, bool ls, int grid, hipStream_t s) {
  TrajArgs a = a0;
  const size_t lds = traj_lds(a);
  static bool attr = false;
  if (!attr) {
    // dynamic LDS above the default 64 KB needs the attribute; the kernels also hold a few hundred bytes
    // of static LDS, so the full 160 KB cannot be requested
    const void* ks[] = {reinterpret_cast<const void*>(&k_traj<false>), reinterpret_cast<const void*>(&k_traj<true>)};
    for (const void* k : ks) {
      (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
      (void)hipGetLastError();
    }
    attr = true;
  }
  if (!ls) hipLaunchKernelGGL(k_traj<false>, dim3(grid), dim3(GMPC_TRAJ_THREADS), lds, s, a);
  else hipLaunchKernelGGL(k_traj<true>, dim3(grid), dim3(GMPC_TRAJ_THREADS), lds, s, a);
}

void gmpc_launch_rollout(const TrajArgs& a0, hipStream_t s) {
  const int grid = (a0.B + GMPC_TB - 1) / GMPC_TB;
  if (gmpc_traj_rw_shape(a0)) {
    TrajArgs a = a0;
    const size_t rlds = gmpc_traj_rw_lds(a);
    gmpc_launch_traj_rw(a, false, grid, rlds, s);
  } else {
    gmpc_launch_traj(a0, false, grid, s);
  }
}

void gmpc_launch_masks(int B, int n, int m, int T, const MlpDesc& dyn, const float* X,
                       const float* U, uint32_t* masks, hipStream_t s) {
  const int NS = B * T;
  const int aw = traj_aw(n, m, dyn, nullptr);
  hipLaunchKernelGGL(k_masks, dim3((NS + 3) / 4), dim3(GMPC_THREADS), 2 * (size_t)aw * sizeof(float4), s,
                     NS, n, m, T, dyn, X, U, masks, aw);
}
