// k_big_step: the per-trajectory pieces of one step of the large-state backward pass (gmpc_large.hip) -- everything
// of the step that is not an n^3 product: linear terms, gains K_t k_t, adjoint, value vector, V = H + G K / 2.
// One workgroup per trajectory.  The kernel is ONE function on purpose: it sits at 256 VGPRs (accum offset 244) with
// no scratch, and splitting it into inlined phase functions -- or only sharing the right-hand-side solve that its two
// gain-solve branches repeat -- keeps the bits and the register counts but reorders a tenth of its instruction
// stream and measured 0.3 - 0.6 % slower at the C5 shape (profiles/EXPERIMENTS.md).  Its phases are marked by the
// "==== phase" banners and the BS_STAMPs between them.
// Reference arithmetic: trajax lqr_step / adjoint (mode 0), the oracle's hessian_solve (mode 1).
#include <type_traits>

#include "gmpc_launch.h"

// 4-row blocks of the matrix-pipe gain solve (big_solve_mfma) for m controls: the instantiated size that holds m
static int big_solve_blocks(int m) { return m <= 8 ? 2 : m <= 20 ? 5 : m <= 32 ? 8 : 16; }
static size_t big_step_lds(int n, int m, int h) {
  const size_t MP = (size_t)((m + 7) & ~7);     // solve columns and the blocked solve's copies are padded to 8
  // the solve's work area: one column per thread + the padded copies of the vector form, or the operand
  // fragments + the padded factor of the matrix-pipe form
  const size_t MB = big_solve_blocks(m), KCH = (4 * MB + 15) / 16;
  const size_t valu = MP * GMPC_THREADS + ((m & 7) ? 3 : 1) * MP * MP + 4, mfma = 3 * MB * KCH * 64 + 16 * MB * MB + 4;
  return ((size_t)2 * m * m + 5 * (size_t)n + 7 * (size_t)m + 16 + 2 * (size_t)h + 2 * GMPC_THREADS +
          (valu > mfma ? valu : mfma)) * sizeof(float);
}

// ------------------------------------------------------------------------------------------------
// [K_t] = -(G + delta I)^-1 H, V = H + G K / 2 of k_big_step (mode 0) with the matrix pipe doing the
// multiply-subtracts.  One column of H per lane as before; the column lives in REGISTERS (y[4 MB]) and is the B
// operand of v_mfma_f32_4x4x1_16B_f32: d[i] += A[i][k] * y[k] for the 4 rows of a block and the lane's own column,
// A = 16 consecutive k of (-L), (-L^T) or G for the block's 4 rows in one VGPR ([k][4 rows] fragments built once
// per trajectory in LDS, broadcast with cbsz / abid as in the trajectory kernels).  What stays on the vector
// pipe is the 4 x 4 triangle on the diagonal of every block (6 multiply-subtracts and 4 divisions per block and
// sweep).  Same operations as the vector form (exact fp32 FMAs, divisions by the diagonal); the multiply-subtracts
// of a row are summed in two interleaved chains (even / odd k) instead of one.
// At the C5 shard (m = 64, n = 1024) the vector form spent 2.3 of k_big_step's 2.8 ms here (0.4 LDS reads per
// multiply-subtract); this form: 2 300 MFMAs of 8 cycles per 64 columns.
// ------------------------------------------------------------------------------------------------
template <int MB>
__device__ __forceinline__ void big_solve_mfma(int n, int m, int nm, const float* L, const float* G,
                                               const float* __restrict__ HG, float* work, float* __restrict__ Kt,
                                               float* __restrict__ KV, float* __restrict__ VK) {
  constexpr int MP = 4 * MB, KCH = (MP + 15) / 16;
  float* const AsF = work;                       // [MB][KCH][16 k][4 rows]: -L below the block's diagonal block
  float* const AsB = AsF + MB * KCH * 64;        // -L^T right of it
  float* const AsG = AsB + MB * KCH * 64;        // G
  float* const Lp = AsG + MB * KCH * 64;         // [MP][MP] L padded with an identity block
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int e = tid; e < MB * KCH * 64; e += GMPC_THREADS) {
    const int l = e & 63, kc = (e >> 6) % KCH, ib = (e >> 6) / KCH;
    const int row = 4 * ib + (l & 3), k = 16 * kc + (l >> 2);
    const bool in = row < m && k < m;
    AsF[e] = (in && k < 4 * ib) ? -L[row * m + k] : 0.f;
    AsB[e] = (in && k >= 4 * ib + 4) ? -L[k * m + row] : 0.f;
    AsG[e] = in ? G[row * m + k] : 0.f;
  }
  for (int e = tid; e < MP * MP; e += GMPC_THREADS) {
    const int i = e / MP, k = e - i * MP;
    Lp[e] = (i < m && k < m) ? L[i * m + k] : (i == k ? 1.f : 0.f);
  }
  __syncthreads();
  const int m_in = m;
  for (int c0 = 0; c0 + 64 * wave < n; c0 += GMPC_THREADS) {          // (uniform per wave: the MFMAs need all lanes)
    // (m made opaque per iteration: the ~200 uniform "row < m" tests below are compared where they are used
    // instead of being hoisted out of the loop into -- and spilled from -- the scalar registers)
    int m = m_in;
    asm volatile("" : "+s"(m));
    const int c = c0 + tid;
    const bool cok = c < n;
    const float* Hc = HG + (cok ? c : n - 1);
    // (rows through walking pointers: 64 loop-invariant row offsets would be hoisted into -- and spilled from --
    // the scalar registers)
    float y[MP];
    {
      const float* hp = Hc;
#pragma unroll
      for (int i = 0; i < MP; ++i) {
        y[i] = i < m ? *hp : 0.f;
        if (i + 1 < m) hp += nm;
      }
    }
    // ---- L y = H: block ib needs y[0 .. 4 ib - 1]
    rw_static_for<MB>([&](auto ibc) __attribute__((always_inline)) {
      constexpr int ib = decltype(ibc)::value;
      f32x4_t d0 = {y[4 * ib], y[4 * ib + 1], y[4 * ib + 2], y[4 * ib + 3]}, d1 = {0.f, 0.f, 0.f, 0.f};
      rw_static_for<(4 * ib + 15) / 16>([&](auto kcc) __attribute__((always_inline)) {
        constexpr int kc = decltype(kcc)::value;
        const float ar = AsF[(ib * KCH + kc) * 64 + lane];
        rw_static_for<16>([&](auto kkc) __attribute__((always_inline)) {
          constexpr int k = 16 * kc + decltype(kkc)::value;
          if constexpr (k < 4 * ib) {
            if constexpr (k & 1) rw_mfma<k>(d1, ar, y[k]);
            else rw_mfma<k>(d0, ar, y[k]);
          }
        });
      });
      const float* Ld = Lp + (4 * ib) * MP + 4 * ib;
      float v0 = d0[0] + d1[0], v1 = d0[1] + d1[1], v2 = d0[2] + d1[2], v3 = d0[3] + d1[3];
      v0 = v0 / Ld[0];
      v1 = (v1 - Ld[MP] * v0) / Ld[MP + 1];
      v2 = ((v2 - Ld[2 * MP] * v0) - Ld[2 * MP + 1] * v1) / Ld[2 * MP + 2];
      v3 = (((v3 - Ld[3 * MP] * v0) - Ld[3 * MP + 1] * v1) - Ld[3 * MP + 2] * v2) / Ld[3 * MP + 3];
      y[4 * ib] = v0; y[4 * ib + 1] = v1; y[4 * ib + 2] = v2; y[4 * ib + 3] = v3;
    });
    // ---- L^T x = y: block ib needs x[4 ib + 4 ..]
    rw_static_for<MB>([&](auto ibr) __attribute__((always_inline)) {
      constexpr int ib = MB - 1 - decltype(ibr)::value;
      f32x4_t d0 = {y[4 * ib], y[4 * ib + 1], y[4 * ib + 2], y[4 * ib + 3]}, d1 = {0.f, 0.f, 0.f, 0.f};
      constexpr int kc0 = (4 * ib + 4) / 16;
      rw_static_for<KCH - kc0>([&](auto kcc) __attribute__((always_inline)) {
        constexpr int kc = kc0 + decltype(kcc)::value;
        const float ar = AsB[(ib * KCH + kc) * 64 + lane];
        rw_static_for<16>([&](auto kkc) __attribute__((always_inline)) {
          constexpr int k = 16 * kc + decltype(kkc)::value;
          if constexpr (k >= 4 * ib + 4 && k < MP) {
            if constexpr (k & 1) rw_mfma<k>(d1, ar, y[k]);
            else rw_mfma<k>(d0, ar, y[k]);
          }
        });
      });
      const float* Ld = Lp + (4 * ib) * MP + 4 * ib;      // U[r][q] = L[q][r]
      float v0 = d0[0] + d1[0], v1 = d0[1] + d1[1], v2 = d0[2] + d1[2], v3 = d0[3] + d1[3];
      v3 = v3 / Ld[3 * MP + 3];
      v2 = (v2 - Ld[3 * MP + 2] * v3) / Ld[2 * MP + 2];
      v1 = ((v1 - Ld[2 * MP + 1] * v2) - Ld[3 * MP + 1] * v3) / Ld[MP + 1];
      v0 = (((v0 - Ld[MP] * v1) - Ld[2 * MP] * v2) - Ld[3 * MP] * v3) / Ld[0];
      y[4 * ib] = v0; y[4 * ib + 1] = v1; y[4 * ib + 2] = v2; y[4 * ib + 3] = v3;
    });
#pragma unroll
    for (int i = 0; i < MP; ++i) y[i] = -y[i];            // K's column
    // ---- V = H + G K / 2, outputs
    const float* hp = Hc;
    const size_t co = cok ? c : 0, mn = (size_t)m * n;
    float* kp = Kt + co;
    float* kvp = KV + co;
    float* vkp = VK + co;
    rw_static_for<MB>([&](auto ibc) __attribute__((always_inline)) {
      constexpr int ib = decltype(ibc)::value;
      f32x4_t d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {0.f, 0.f, 0.f, 0.f};
      float hr[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        hr[r] = 4 * ib + r < m ? *hp : 0.f;
        if (4 * ib + r + 1 < m) hp += nm;
      }
      rw_static_for<KCH>([&](auto kcc) __attribute__((always_inline)) {
        constexpr int kc = decltype(kcc)::value;
        const float ar = AsG[(ib * KCH + kc) * 64 + lane];
        rw_static_for<16>([&](auto kkc) __attribute__((always_inline)) {
          constexpr int k = 16 * kc + decltype(kkc)::value;
          if constexpr (k < MP) {
            if constexpr (k & 1) rw_mfma<k>(d1, ar, y[k]);
            else rw_mfma<k>(d0, ar, y[k]);
          }
        });
      });
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 4 * ib + r;
        if (i < m && cok) {
          const float kic = y[i];
          const float vic = fmaf(0.5f, d0[r] + d1[r], hr[r]);
          *kp = kic;
          *kvp = kic;
          kvp[mn] = vic;
          *vkp = vic;
          vkp[mn] = kic;
        }
        kp += n; kvp += n; vkp += n;
      }
    });
  }
}

#ifdef GMPC_BIGSTEP_STAMPS
#define BS_STAMP(i) { __syncthreads(); if (threadIdx.x == 0) bs_t[i] = __builtin_readcyclecounter(); }
#else
#define BS_STAMP(i)
#endif
__global__ __launch_bounds__(GMPC_THREADS) void k_big_step(BigStepArgs a) {
#ifdef GMPC_BIGSTEP_STAMPS
  unsigned long long bs_t[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  BS_STAMP(0)
#endif
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int n = a.n, m = a.m, T = a.T, t = a.t, nm = n + m;
  const int tid = threadIdx.x, b = blockIdx.x;
  if (a.active != nullptr && a.active[b] == 0) return;
  float* G = reinterpret_cast<float*>(smem);     // m x m  (symmetrised R + B^T P B)
  float* L = G + m * m;                          // m x m  Cholesky factor / work copy
  float* pv = L + m * m;                         // n
  float* lv = pv + n;                            // n
  float* dv = lv + n;                            // n   x - goal
  float* qv = dv + n;                            // n
  float* pa = qv + n;                            // n   A^T p
  float* uv = pa + n;                            // m
  float* rv = uv + m;                            // m
  float* hv = rv + m;                            // m
  float* kv = hv + m;                            // m
  float* gk = kv + m;                            // m   G k + h
  float* gsq = gk + m;                           // m
  int* perm = reinterpret_cast<int*>(gsq + m);   // m   row permutation of the LU (mode 1)
  float* red = gsq + 2 * m;                      // 16
  float* yl = red + 16;                          // h   W_L lam   (low-rank form)
  float* yp = yl + a.h;                          // h   W_L p
  float* part = yp + a.h;                        // 2 x 256 partial sums
  float* ycol = part + 2 * GMPC_THREADS;         // m x 256: one solve column per thread
  const float* AB = a.ABt + (size_t)b * n * nm;
  const float* HG = a.HG + (size_t)b * m * nm;
  const size_t bt = (size_t)b * T + t;
  // ==== phase: load: x - goal, u, p and lam of step t + 1; the linear terms q, r =================================
  const float w0 = sigmoidf_(a.mpc_w[0]), w1 = sigmoidf_(a.mpc_w[1]);
  const float al = GMPC_ALPHA;
  float dd = 0.f, uu = 0.f;
  const int ng = a.ng > 0 ? a.ng : n;      // the staging cost sees xc[:ng]
  for (int i = tid; i < n; i += blockDim.x) {
    const size_t xi = ((size_t)b * (T + 1) + t) * n + i;
    const float d = i < ng ? a.X[xi] - a.goal[((size_t)b * (T + 1) + t) * ng + i] : 0.f;
    dv[i] = d;
    dd = fmaf(d, d, dd);
    pv[i] = a.pvec[(size_t)b * n + i];
    lv[i] = a.lam[(size_t)b * n + i];
  }
  for (int j = tid; j < m; j += blockDim.x) {
    const float u = a.U[bt * m + j];
    uv[j] = u;
    uu = fmaf(u, u, uu);
  }
  dd = wave_sum(dd); uu = wave_sum(uu);
  if ((tid & 63) == 0) { red[tid >> 6] = dd; red[4 + (tid >> 6)] = uu; }
  __syncthreads();
  dd = (red[0] + red[1]) + (red[2] + red[3]);
  uu = (red[4] + red[5]) + (red[6] + red[7]);
  const float s = sqrtf(dd + al * al), su = sqrtf(uu + al * al);
  const float isu = 1.f / su, isu3 = 1.f / (su * su * su);
  if (tid == 0) a.sbuf[b] = s;
  // linear terms of the two vector recursions: mode 0 the cost gradient (q_t, r_t) for both the
  // adjoint lambda and the value vector p; mode 1 (d loss/d x_t, d loss/d u_t or 0) for the loss adjoint and
  // (0, -Bvec_t) for p
  const bool m1 = a.mode == 1;
  for (int i = tid; i < n; i += blockDim.x)
    qv[i] = m1 ? a.lx[((size_t)b * (T + 1) + t) * n + i] : w1 * dv[i] / s;
  for (int j = tid; j < m; j += blockDim.x)
    rv[j] = m1 ? (a.lu != nullptr ? a.lu[bt * m + j] : 0.f) : w0 * uv[j] / su;
  __syncthreads();
  BS_STAMP(1)
  // ==== phase: low-rank form: yl = W_L lam, yp = W_L p ===========================================================
  const bool lowrank = a.Vt != nullptr;
  const float* Vt = lowrank ? a.Vt + (size_t)b * a.h * nm : nullptr;
  if (lowrank) {
    // y = W_L v for v = lam, p: one wave per row of W_L (coalesced along the row), four rows and four 64-wide
    // slices at a time so that 16 loads are in flight (one load per iteration left every one of the 16 k
    // loads of a wave's rows exposed: 0.68 M of the kernel's 2.8 M cycles at n = 1024, h = 200)
    const int wave = tid >> 6, ln = tid & 63;
    constexpr int NW = GMPC_THREADS / 64, RW = 4;       // rows per wave and pass: 16 loads in flight
    for (int k = wave; k < a.h; k += RW * NW) {
      const float* wr[RW];
      bool ok[RW];
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        ok[r] = k + r * NW < a.h;
        wr[r] = a.WL + (size_t)(ok[r] ? k + r * NW : k) * n;
      }
      float sl[RW], sp[RW];
#pragma unroll
      for (int r = 0; r < RW; ++r) { sl[r] = 0.f; sp[r] = 0.f; }
      for (int i0 = ln; i0 < n; i0 += 256) {
        float wv[RW][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = min(i0 + 64 * q, n - 1);
#pragma unroll
          for (int r = 0; r < RW; ++r) wv[r][q] = wr[r][i];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = i0 + 64 * q;
          const float lvi = i < n ? lv[i] : 0.f, pvi = i < n ? pv[i] : 0.f;
#pragma unroll
          for (int r = 0; r < RW; ++r) { sl[r] = fmaf(wv[r][q], lvi, sl[r]); sp[r] = fmaf(wv[r][q], pvi, sp[r]); }
        }
      }
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        const float a_ = wave_sum(sl[r]), b_ = wave_sum(sp[r]);
        if (ln == 0 && ok[r]) { yl[k + r * NW] = a_; yp[k + r * NW] = b_; }
      }
    }
    __syncthreads();
  }
  BS_STAMP(2)
  // ==== phase: g, h ==============================================================================================
  // g_t = r + B^T lam ; h = r + B^T p : thread (rp, j) sums rows rp, rp + RP, ... of column j of B
  // (low-rank form: B^T v = Vu (W_L v), rows of V^T instead of rows of B)
  {
    const int MC = m <= 32 ? 32 : 64, RP = GMPC_THREADS / MC;
    const int rp = tid / MC, j = tid - rp * MC;
    float g = 0.f, h = 0.f;
    if (j < m) {
      // (8 loads in flight; the sums keep the order of the one-load loop)
      const float* Mj = (lowrank ? Vt : AB) + n + j;
      const float* vL = lowrank ? yl : lv;
      const float* vP = lowrank ? yp : pv;
      const int rows = lowrank ? a.h : n;
      int i = rp;
      for (; i + 7 * RP < rows; i += 8 * RP) {
        float e[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) e[r] = Mj[(size_t)(i + r * RP) * nm];
#pragma unroll
        for (int r = 0; r < 8; ++r) { g = fmaf(e[r], vL[i + r * RP], g); h = fmaf(e[r], vP[i + r * RP], h); }
      }
      for (; i < rows; i += RP) {
        const float e = Mj[(size_t)i * nm];
        g = fmaf(e, vL[i], g);
        h = fmaf(e, vP[i], h);
      }
    }
    part[tid] = g;
    part[GMPC_THREADS + tid] = h;
    __syncthreads();
    if (tid < m) {
      float gs = 0.f, hs = 0.f;
      for (int r = 0; r < RP; ++r) { gs += part[r * MC + tid]; hs += part[GMPC_THREADS + r * MC + tid]; }
      gs = rv[tid] + gs;
      if (m1) {
        a.Bvec[bt * m + tid] = gs;          // B_t^T mu_{t+1} (+ lu_t)
        hv[tid] = hs - gs;                  // h = -Bvec_t + B^T p
      } else {
        hv[tid] = rv[tid] + hs;
        a.grad[bt * m + tid] = gs;
      }
      gsq[tid] = gs * gs;
    }
  }
  BS_STAMP(3)
  // ==== phase: lam, pa ===========================================================================================
  // lam_t = q + A^T lam ; pa = A^T p: column c of A is read coalesced across threads, NQ columns of a thread and RI
  // rows at a time -- 16 loads in flight.  NQ follows n (four columns per thread at n = 376 made 2.7 loads per useful
  // one: the clamped duplicates of columns past n); the sums run over the rows in the same order whatever RI is.
  {
    const float* M = lowrank ? Vt : AB;
    const float* vL = lowrank ? yl : lv;
    const float* vP = lowrank ? yp : pv;
    const int rows = lowrank ? a.h : n;
    auto matvec = [&](auto nqc, auto ric) __attribute__((always_inline)) {
      constexpr int NQ = decltype(nqc)::value, RI = decltype(ric)::value;
      for (int c0 = tid; c0 < n; c0 += NQ * (int)blockDim.x) {
        float vl[NQ], vp[NQ];
        int cq[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) { vl[q] = 0.f; vp[q] = 0.f; cq[q] = min(c0 + q * (int)blockDim.x, n - 1); }
        int i = 0;
        for (; i + RI <= rows; i += RI) {
          float e[RI][NQ], lr[RI], pr[RI];
#pragma unroll
          for (int r = 0; r < RI; ++r) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) e[r][q] = M[(size_t)(i + r) * nm + cq[q]];
            lr[r] = vL[i + r];
            pr[r] = vP[i + r];
          }
#pragma unroll
          for (int r = 0; r < RI; ++r)
#pragma unroll
            for (int q = 0; q < NQ; ++q) { vl[q] = fmaf(e[r][q], lr[r], vl[q]); vp[q] = fmaf(e[r][q], pr[r], vp[q]); }
        }
        for (; i < rows; ++i) {
#pragma unroll
          for (int q = 0; q < NQ; ++q) {
            const float ev = M[(size_t)i * nm + cq[q]];
            vl[q] = fmaf(ev, vL[i], vl[q]); vp[q] = fmaf(ev, vP[i], vp[q]);
          }
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const int c = c0 + q * (int)blockDim.x;
          if (c >= n) continue;
          if (lowrank) { vl[q] += lv[c]; vp[q] += pv[c]; }      // A^T v = v + Vx (W_L v)
          pa[c] = vp[q];
          const float ln = qv[c] + vl[q];
          a.lam[(size_t)b * n + c] = ln;
          if (!m1) a.adj[((size_t)b * (T + 1) + t) * n + c] = ln;
        }
      }
    };
    const int nq = (n + (int)blockDim.x - 1) / (int)blockDim.x;
    if (nq <= 1) matvec(std::integral_constant<int, 1>{}, std::integral_constant<int, 16>{});
    else if (nq == 2) matvec(std::integral_constant<int, 2>{}, std::integral_constant<int, 8>{});
    else matvec(std::integral_constant<int, 4>{}, std::integral_constant<int, 4>{});
  }
  BS_STAMP(4)
  // ==== phase: G =================================================================================================
  // G = sym(R + B^T P B)
  for (int e = tid; e < m * m; e += blockDim.x) {
    const int i = e / m, j = e - i * m;
    const float Rij = w0 * ((i == j ? isu : 0.f) - uv[i] * uv[j] * isu3);
    L[e] = Rij + HG[(size_t)i * nm + n + j];
  }
  __syncthreads();
  if (tid == 0 && !m1) {
    float sg = 0.f;
    for (int j = 0; j < m; ++j) sg += gsq[j];
    a.gn2[b] += sg;
  }
  for (int e = tid; e < m * m; e += blockDim.x) {
    const int i = e / m, j = e - i * m;
    G[e] = (L[e] + L[j * m + i]) * 0.5f;
  }
  __syncthreads();
  float* Kt = a.K + bt * m * n;
  float* KV = a.KV + (size_t)b * 2 * m * n;
  float* VK = a.VK + (size_t)b * 2 * m * n;
  float* y = ycol + tid;
  if (!m1) {
    BS_STAMP(5)
    // ==== phase: Cholesky ========================================================================================
    // Cholesky of G + 1e-8 I in L (lower), column by column; NaN on a non-positive pivot
    for (int e = tid; e < m * m; e += blockDim.x) L[e] = G[e] + ((e / m) == (e % m) ? 1e-8f : 0.f);
    __syncthreads();
    for (int j = 0; j < m; ++j) {
      if (tid == 0) L[j * m + j] = sqrtf(L[j * m + j]);
      __syncthreads();
      const float d = L[j * m + j];
      for (int i = j + 1 + tid; i < m; i += blockDim.x) L[i * m + j] /= d;
      __syncthreads();
      // trailing update of the lower triangle: L[i][k] -= L[i][j] L[k][j], j < k <= i; thread (tid / 16, tid % 16)
      // walks rows and columns in steps of 16 (no integer division by the shrinking size in the loop)
      for (int i = j + 1 + (tid >> 4); i < m; i += GMPC_THREADS / 16) {
        const float lij = L[i * m + j];
        for (int k = j + 1 + (tid & 15); k <= i; k += 16) L[i * m + k] -= lij * L[k * m + j];
      }
      __syncthreads();
    }
    BS_STAMP(6)
    // ==== phase: gain solve: matrix-pipe form, else vector form ==================================================
    // [K k] = -(G + delta I)^-1 [H h]
    if (!a.solve_valu && m <= 64) {
      // the right-hand side h: wave 0 across its lanes (see the vector form below); the n columns of H: one
      // per lane, the multiply-subtracts on the matrix pipe (big_solve_mfma)
      if (tid < 64) {
        float v = tid < m ? hv[tid] : 0.f, yv = 0.f;
        for (int k = 0; k < m; ++k) {
          const float yk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)) / L[k * m + k];
          if (tid == k) yv = yk;
          if (tid > k && tid < m) v -= L[tid * m + k] * yk;
        }
        for (int k = m - 1; k >= 0; --k) {
          const float xk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(yv), k)) / L[k * m + k];
          if (tid == k) yv = xk;
          if (tid < k) yv -= L[k * m + tid] * xk;
        }
        if (tid < m) { kv[tid] = -yv; a.k[bt * m + tid] = -yv; }
      }
      if (m <= 8) big_solve_mfma<2>(n, m, nm, L, G, HG, ycol, Kt, KV, VK);
      else if (m <= 20) big_solve_mfma<5>(n, m, nm, L, G, HG, ycol, Kt, KV, VK);
      else if (m <= 32) big_solve_mfma<8>(n, m, nm, L, G, HG, ycol, Kt, KV, VK);
      else big_solve_mfma<16>(n, m, nm, L, G, HG, ycol, Kt, KV, VK);
    } else
    // the vector form: one right-hand-side column per thread (column n is h); the thread keeps its column in
    // LDS (ycol[i][tid])
    {
      // blocks of 8 rows share the loads of the solved part of the column and read their rows of L (L^T in
      // the backward sweep) and G 16 bytes at a time -- 0.4 LDS reads per multiply-subtract instead of 2 (the
      // scalar form spent 9.4 ms per time step of the C5 shard in this loop).  m is padded to a multiple of
      // 8 with an identity block (copies Lb / Ltb / Gb with row stride MP; for m % 8 == 0 L and G are used in
      // place and only the transpose is built)
      const int MP = (m + 7) & ~7;
      float* xtra = reinterpret_cast<float*>(
          (reinterpret_cast<uintptr_t>(ycol + (size_t)MP * GMPC_THREADS) + 15) & ~(uintptr_t)15);
      float* Ltb = xtra;                                    // Ltb[i][k] = L[k][i]
      float* Lb = (m & 7) ? xtra + MP * MP : L;
      float* Gb = (m & 7) ? xtra + 2 * MP * MP : G;
      for (int e = tid; e < MP * MP; e += blockDim.x) {
        const int i = e / MP, k = e - i * MP;
        const bool in = i < m && k < m;
        Ltb[e] = in ? L[k * m + i] : (i == k ? 1.f : 0.f);
        if (m & 7) {
          Lb[e] = in ? L[i * m + k] : (i == k ? 1.f : 0.f);
          Gb[e] = in ? G[i * m + k] : 0.f;
        }
      }
      __syncthreads();
      // the right-hand side h (column n): one more column would be one more sweep of the loop below for a
      // single thread (n = 1024: a fifth sweep as long as the other four) -- wave 0 solves it across its lanes
      // instead, lane i = row i, the pivot's value handed round with v_readlane
      const bool hwave = m <= 64;
      if (hwave && tid < 64) {
        float v = tid < m ? hv[tid] : 0.f, yv = 0.f;
        for (int k = 0; k < m; ++k) {
          const float yk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)) / L[k * m + k];
          if (tid == k) yv = yk;
          if (tid > k && tid < m) v -= L[tid * m + k] * yk;
        }
        for (int k = m - 1; k >= 0; --k) {
          const float xk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(yv), k)) / L[k * m + k];
          if (tid == k) yv = xk;
          if (tid < k) yv -= L[k * m + tid] * xk;
        }
        if (tid < m) { kv[tid] = -yv; a.k[bt * m + tid] = -yv; }
      }
      for (int c = tid; c < n + (hwave ? 0 : 1); c += blockDim.x) {
        for (int i0 = 0; i0 < MP; i0 += 8) {
          float acc[8], yb[8];
#pragma unroll
          for (int r = 0; r < 8; ++r)
            acc[r] = i0 + r < m ? (c < n ? HG[(size_t)(i0 + r) * nm + c] : hv[i0 + r]) : 0.f;
          for (int k = 0; k < i0; k += 4) {
            const float y0 = y[(k + 0) * GMPC_THREADS], y1 = y[(k + 1) * GMPC_THREADS];
            const float y2 = y[(k + 2) * GMPC_THREADS], y3 = y[(k + 3) * GMPC_THREADS];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
              const float4 l4 = *reinterpret_cast<const float4*>(&Lb[(i0 + r) * MP + k]);
              acc[r] -= l4.x * y0; acc[r] -= l4.y * y1; acc[r] -= l4.z * y2; acc[r] -= l4.w * y3;
            }
          }
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            float v = acc[r];
#pragma unroll
            for (int q = 0; q < r; ++q) v -= Lb[(i0 + r) * MP + i0 + q] * yb[q];
            yb[r] = v / Lb[(i0 + r) * MP + i0 + r];
            y[(i0 + r) * GMPC_THREADS] = yb[r];
          }
        }
        for (int i0 = MP - 8; i0 >= 0; i0 -= 8) {
          float acc[8], xb[8];
#pragma unroll
          for (int r = 0; r < 8; ++r) acc[r] = y[(i0 + r) * GMPC_THREADS];
          for (int k = i0 + 8; k < MP; k += 4) {
            const float y0 = y[(k + 0) * GMPC_THREADS], y1 = y[(k + 1) * GMPC_THREADS];
            const float y2 = y[(k + 2) * GMPC_THREADS], y3 = y[(k + 3) * GMPC_THREADS];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
              const float4 l4 = *reinterpret_cast<const float4*>(&Ltb[(i0 + r) * MP + k]);
              acc[r] -= l4.x * y0; acc[r] -= l4.y * y1; acc[r] -= l4.z * y2; acc[r] -= l4.w * y3;
            }
          }
#pragma unroll
          for (int r = 7; r >= 0; --r) {
            float v = acc[r];
#pragma unroll
            for (int q = r + 1; q < 8; ++q) v -= Ltb[(i0 + r) * MP + i0 + q] * xb[q];
            xb[r] = v / Lb[(i0 + r) * MP + i0 + r];
            y[(i0 + r) * GMPC_THREADS] = xb[r];
          }
        }
        if (c < n) {
          for (int i0 = 0; i0 < MP; i0 += 8) {
            float acc[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) acc[r] = 0.f;
            for (int k = 0; k < MP; k += 4) {
              const float y0 = -y[(k + 0) * GMPC_THREADS], y1 = -y[(k + 1) * GMPC_THREADS];
              const float y2 = -y[(k + 2) * GMPC_THREADS], y3 = -y[(k + 3) * GMPC_THREADS];
#pragma unroll
              for (int r = 0; r < 8; ++r) {
                const float4 g4 = *reinterpret_cast<const float4*>(&Gb[(i0 + r) * MP + k]);
                acc[r] = fmaf(g4.x, y0, acc[r]); acc[r] = fmaf(g4.y, y1, acc[r]);
                acc[r] = fmaf(g4.z, y2, acc[r]); acc[r] = fmaf(g4.w, y3, acc[r]);
              }
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) {
              const int i = i0 + r;
              if (i >= m) continue;
              const float kic = -y[i * GMPC_THREADS];
              const float vic = fmaf(0.5f, acc[r], HG[(size_t)i * nm + c]);
              Kt[(size_t)i * n + c] = kic;
              KV[(size_t)i * n + c] = kic;
              KV[(size_t)(m + i) * n + c] = vic;
              VK[(size_t)i * n + c] = vic;
              VK[(size_t)(m + i) * n + c] = kic;
            }
          }
        } else {
          for (int i = 0; i < m; ++i) { kv[i] = -y[i * GMPC_THREADS]; a.k[bt * m + i] = -y[i * GMPC_THREADS]; }
        }
      }
    }
  } else {
    // ==== phase: mode 1: LU solve ================================================================================
    // LU with partial pivoting (jax.scipy.linalg.solve as the reference calls it), in place in L:
    // unit-lower multipliers below the diagonal, U on and above; perm = row order
    for (int e = tid; e < m * m; e += blockDim.x) L[e] = G[e];
    for (int i = tid; i < m; i += blockDim.x) perm[i] = i;
    __syncthreads();
    for (int j = 0; j < m; ++j) {
      if (tid == 0) {
        int piv = j;
        float best = fabsf(L[j * m + j]);
        for (int i = j + 1; i < m; ++i)
          if (fabsf(L[i * m + j]) > best) { best = fabsf(L[i * m + j]); piv = i; }
        red[0] = (float)piv;
        if (piv != j) { const int tp = perm[j]; perm[j] = perm[piv]; perm[piv] = tp; }
      }
      __syncthreads();
      const int piv = (int)red[0];
      if (piv != j)
        for (int c = tid; c < m; c += blockDim.x) {
          const float tv_ = L[j * m + c]; L[j * m + c] = L[piv * m + c]; L[piv * m + c] = tv_;
        }
      __syncthreads();
      const float d = L[j * m + j];
      for (int i = j + 1 + tid; i < m; i += blockDim.x) L[i * m + j] /= d;
      __syncthreads();
      const int rem = m - j - 1;
      for (int e = tid; e < rem * rem; e += blockDim.x) {
        const int i = j + 1 + e / rem, k = j + 1 + e % rem;
        L[i * m + k] -= L[i * m + j] * L[j * m + k];
      }
      __syncthreads();
    }
    for (int c = tid; c <= n; c += blockDim.x) {
      for (int i = 0; i < m; ++i) {
        const int pi = perm[i];
        float v = c < n ? HG[(size_t)pi * nm + c] : hv[pi];
        for (int k = 0; k < i; ++k) v -= L[i * m + k] * y[k * GMPC_THREADS];
        y[i * GMPC_THREADS] = v;
      }
      for (int i = m - 1; i >= 0; --i) {
        float v = y[i * GMPC_THREADS];
        for (int k = i + 1; k < m; ++k) v -= L[i * m + k] * y[k * GMPC_THREADS];
        y[i * GMPC_THREADS] = v / L[i * m + i];
      }
      if (c < n) {
        // K column, V = H + G K / 2 and the stacked operands [K; V], [V; K] of the cross-term product
        // (the column is still in LDS: no global re-reads)
        for (int i = 0; i < m; ++i) {
          float v = 0.f;
          for (int k = 0; k < m; ++k) v = fmaf(G[i * m + k], -y[k * GMPC_THREADS], v);
          const float kic = -y[i * GMPC_THREADS];
          const float vic = fmaf(0.5f, v, HG[(size_t)i * nm + c]);
          Kt[(size_t)i * n + c] = kic;
          KV[(size_t)i * n + c] = kic;
          KV[(size_t)(m + i) * n + c] = vic;
          VK[(size_t)i * n + c] = vic;
          VK[(size_t)(m + i) * n + c] = kic;
        }
      } else {
        for (int i = 0; i < m; ++i) { kv[i] = -y[i * GMPC_THREADS]; a.k[bt * m + i] = -y[i * GMPC_THREADS]; }
      }
    }
  }
  BS_STAMP(7)
  // ==== phase: G k + h and p =====================================================================================
  __syncthreads();
  for (int i = tid; i < m; i += blockDim.x) {
    float v = 0.f;
    for (int k = 0; k < m; ++k) v = fmaf(G[i * m + k], kv[k], v);
    gk[i] = v + hv[i];
  }
  __syncthreads();
  // p = q + A^T p + H^T k + K^T (G k + h)      [= q + A^T p + (H+GK)^T k + K^T h, G symmetric]
  for (int c = tid; c < n; c += blockDim.x) {
    float v1 = 0.f, v2 = 0.f;
    // (eight rows at a time -- 16 loads in flight -- measured slower: 99 k vs 86 k cycles at the C5 shard)
    for (int i = 0; i < m; ++i) {
      v1 = fmaf(HG[(size_t)i * nm + c], kv[i], v1);
      v2 = fmaf(Kt[(size_t)i * n + c], gk[i], v2);   // own column: written by this thread above
    }
    a.pvec[(size_t)b * n + c] = (((m1 ? 0.f : qv[c]) + pa[c]) + v1) + v2;
  }
#ifdef GMPC_BIGSTEP_STAMPS
  BS_STAMP(8)
  if (blockIdx.x == 0 && threadIdx.x == 0 && a.t == a.T - 2)
    printf("k_big_step cycles: load %llu | y=WL v %llu | g,h %llu | lam,pa %llu | G %llu | chol %llu | solve %llu | gk,p %llu | total %llu\n",
           bs_t[1] - bs_t[0], bs_t[2] - bs_t[1], bs_t[3] - bs_t[2], bs_t[4] - bs_t[3], bs_t[5] - bs_t[4], bs_t[6] - bs_t[5],
           bs_t[7] - bs_t[6], bs_t[8] - bs_t[7], bs_t[8] - bs_t[0]);
#endif
}

int gmpc_launch_big_step(const BigStepArgs& a, hipStream_t s) {
  const size_t lds = big_step_lds(a.n, a.m, a.h);
  if (lds > 159 * 1024) return -2;     // one workgroup per CU may take (almost) all of the 160 KB
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_big_step),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipGetLastError();
    attr = true;
  }
  hipLaunchKernelGGL(k_big_step, dim3(a.B), dim3(GMPC_THREADS), lds, s, a);
  return 0;
}
