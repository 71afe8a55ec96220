// What the sampling solvers' kernels share beyond the sampler: the sampled rollout -- one body (cem_rollout_body), one
// kernel template around it (k_sampled_rollout) and one launcher (sampled_launch_rollout), each instantiated over where
// a row's controls come from (CemDrawn of gmpc_cem.hip, IcemDrawn of gmpc_icem.hip) -- and the (cost, row) keys with
// their sort (k_cem_update, k_icem_update).
#pragma once
#include "gmpc_dg_gemm.h"
#include "gmpc_cem_sampler.h"

#define GMPC_CEM_ROWS 32          // samples per workgroup of the rollout (the two row halves of dg_gemm)
// LDS of the rollout's operand blocks, in bytes: the fp32 block [32][GMPC_DG_LDA]; in bf16 mode the bf16 block
// [32][GMPC_DG_LDH] behind it (33,280 + 16,896 = 50,176: three workgroups per compute unit, as the registers allow)
#define GMPC_CEM_LDS32 (GMPC_CEM_ROWS * GMPC_DG_LDA * 4)
#define GMPC_CEM_LDS16 (GMPC_CEM_LDS32 + GMPC_CEM_ROWS * GMPC_DG_LDH * 2)
#define GMPC_SAMPLED_LDS_BYTES 65536     // dynamic LDS a launch may ask for without opting in to more

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

// The bf16 mode's stores.  Columns 0 .. Kp-1 of the 32 rows of the bf16 operand block Hb, f's
// values rounded to bf16 (to nearest even; a NaN stays one) in columns below N and zeros from N on -- the k-tail a
// product pads to, whatever a wider layer left there; with F32 also the fp32 values into columns 0 .. N-1 of Ab
// (what the cost terms read); without H16 only those.
template <bool F32, bool H16, typename F>
__device__ __forceinline__ void cem_store_tiles16(float* Ab, __bf16* Hb, const DgTiles& v, int N, int Kp, int wave,
                                                  int lane, F f) {
  const int l16 = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int ci = 0; ci < 4; ++ci) {
    const int j = (wave + 4 * ci) * 16 + l16;
    if (j >= Kp) continue;
    const bool in = j < N;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const float x = in ? f(v.p[ci][rr], j) : 0.f, y = in ? f(v.q[ci][rr], j) : 0.f;
      if constexpr (H16) {
        Hb[(4 * kq + rr) * GMPC_DG_LDH + j] = static_cast<__bf16>(x);
        Hb[(16 + 4 * kq + rr) * GMPC_DG_LDH + j] = static_cast<__bf16>(y);
      }
      if constexpr (F32) {
        if (in) {
          Ab[(4 * kq + rr) * GMPC_DG_LDA + j] = x;
          Ab[(16 + 4 * kq + rr) * GMPC_DG_LDA + j] = y;
        }
      }
    }
  }
}

// One 256-thread workgroup per 32 rows of one problem, the whole horizon.  `rows` rows per problem, costs [B][ldc];
// Ab: the [32][GMPC_DG_LDA] operand block at the start of the dynamic LDS.  Src, where the controls come from.  What
// the body asks of it:
//   begin(b, s0, tid)         once, before the first step (it may fill LDS behind the operand blocks and synchronise)
//   control(b, i, s, t, j)    the control j of step t of row s = s0 + i of problem b
//   record(b, s, t, j, u)     the debug copy of that control, if the caller asked for one
// and what the kernel template and the launcher ask of it (static, host and device, over its arguments Src::Args):
//   roll(a) / rows(a) / ldc(a)   the CemRollArgs inside a, the rows per problem, the stride of the costs
//   Src(a, behind)            `behind`: the dynamic LDS behind the operand block or blocks
//   plan(a, blocks, &extra)   host only: non-zero when the launcher refuses a; otherwise a's launch-time fields are set
//                             and extra is the bytes of LDS the source wants behind the `blocks` bytes of operands
// A row's cost is a function of its controls alone: not of its place in the tile, of `rows` or of B.
// Ens, which dynamics network the workgroup rolls its rows out under and where their costs go:
//   step(t)                   once per step, ahead of its layers: the step's member index (0 where the step plays no part)
//   W(w, p) / b(v, p)         a dynamics layer's weights / biases under step()'s p, from the bound descriptor's pointers
//   costs(c)                  the [B][ldc] plane the rows' costs are written to
//   records()                 whether this workgroup writes the debug copy of the controls
// CemOneModel: the arguments' own network and cost buffer (every kernel without an ensemble).  It and CemMember ignore
// the step; CemParticle draws its member in step().  CemDisagree is
// CemMember with a second, nominal network: its steps are cem_disagree_step's.
// BF16: the layer inputs are rounded to bf16 into Hb, the [32][GMPC_DG_LDH] block behind Ab,
// the layers run on dg_gemm_bf16, and dyn.W[l] / cost.W[l] point at the layers' packed bf16 images (dg_kp, dg_np);
// Ab keeps the fp32 [x_t; u_t] and the last cost layer's output, which the cost terms read as before.  Without BF16
// Hb is not used.
struct CemOneModel {
  static constexpr bool disagree = false;
  __device__ __forceinline__ uint32_t step(int) const { return 0; }
  __device__ __forceinline__ const float* W(const float* w, uint32_t) const { return w; }
  __device__ __forceinline__ const float* b(const float* v, uint32_t) const { return v; }
  __device__ __forceinline__ float* costs(float* c) const { return c; }
  __device__ __forceinline__ bool records() const { return true; }
};

// The member blockIdx.y of a dynamics ensemble: the arguments' dyn describes member 0, member p lies wstride / bstride
// floats behind it (fp32 mode: both the members' parameter count; bf16 mode: W[l] are bf16 images, wstride half their
// elements, the biases stay in the fp32 members), and its costs go to plane p of part [P][B][ldc].
struct CemMember {
  static constexpr bool disagree = false;
  size_t wstride, bstride, plane;
  float* part;
  __device__ __forceinline__ uint32_t step(int) const { return 0; }
  __device__ __forceinline__ const float* W(const float* w, uint32_t) const { return w + blockIdx.y * wstride; }
  __device__ __forceinline__ const float* b(const float* v, uint32_t) const { return v + blockIdx.y * bstride; }
  __device__ __forceinline__ float* costs(float*) const { return part + blockIdx.y * plane; }
  __device__ __forceinline__ bool records() const { return blockIdx.y == 0; }
};

// The particle blockIdx.y of the TS1 propagation: CemMember's strides and planes, but the
// member is drawn anew at every step t, member = umulhi(philox(t, particle, 0xFFFFFFFF, it)[0], P) under the launch's
// key.  Counter word 2 is the problem index in every normal draw (below max_batch), so 0xFFFFFFFF is a stream of its
// own.  Nothing of the draw depends on the row, the tile or the problem: every workgroup of a grid row runs the same
// member sequence (one weight operand per tile of 32 rows), and the draw is uniform over the workgroup --
// evaluated by step(), once per step (W and b of the step's layers take its result), and read back as a scalar, so the
// layers' pointers stay in scalar registers as CemMember's do.  Its costs go to plane `particle` of part [Q][B][ldc].
struct CemParticle {
  static constexpr bool disagree = false;
  size_t wstride, bstride, plane;
  float* part;
  uint32_t P, key0, key1, it;
  __device__ __forceinline__ uint32_t step(int t) const {
    uint32_t r[4];
    cem_philox((uint32_t)t, blockIdx.y, 0xFFFFFFFFu, it, key0, key1, r);
    return __builtin_amdgcn_readfirstlane(__umulhi(r[0], P));
  }
  __device__ __forceinline__ const float* W(const float* w, uint32_t p) const { return w + p * wstride; }
  __device__ __forceinline__ const float* b(const float* v, uint32_t p) const { return v + p * bstride; }
  __device__ __forceinline__ float* costs(float*) const { return part + blockIdx.y * plane; }
  __device__ __forceinline__ bool records() const { return blockIdx.y == 0; }
};

// The one-step disagreement of member blockIdx.y with the nominal model: CemMember's strides and
// planes for the member, `nom` for the nominal layers -- the context's bound dynamics (bf16 mode: W[l] at their packed
// images), which the rows are rolled out under.  The plane's cost is the nominal cost plus penalty times the summed
// squared deviation of the member's one-step output along the nominal rollout.
struct CemDisagree {
  static constexpr bool disagree = true;
  size_t wstride, bstride, plane;
  float* part;
  CemNominal nom;
  float penalty;
  __device__ __forceinline__ uint32_t step(int) const { return 0; }
  __device__ __forceinline__ const float* W(const float* w, uint32_t) const { return w + blockIdx.y * wstride; }
  __device__ __forceinline__ const float* b(const float* v, uint32_t) const { return v + blockIdx.y * bstride; }
  __device__ __forceinline__ const CemNominal& nominal() const { return nom; }
  __device__ __forceinline__ float* costs(float*) const { return part + blockIdx.y * plane; }
  __device__ __forceinline__ bool records() const { return blockIdx.y == 0; }
};

// J + penalty D as two IEEE fp32 operations (the product rounded before it is added), so NumPy restates a plane's cost
// from J and D bit for bit
__device__ __forceinline__ float cem_penalised(float J, float penalty, float D) {
#pragma clang fp contract(off)
  const float pd = penalty * D;
  return J + pd;
}

// One step of a disagreement rollout, the one copy of its arithmetic (k_sampled_rollout under CemDisagree and
// k_ens_disagreement call it).  On entry the operand block holds the layer-0 input [x_t; u_t] of the 32 rows (bf16
// mode: Hb), synchronised; xs is x_t.  Both networks' layer-0 products are taken from that input before anything
// overwrites it, so it is neither saved nor formed twice; then the member's remaining layers run (pass 0), its output
// o^p = acc + bias staying in registers, then the nominal's (pass 1: the same loop body, one copy of the products in
// the code), o^0 formed by the same operations on the same kind of operands -- a member equal to the nominal layers
// gives o^p - o^0 == 0 exactly.  The difference goes through Ab (columns 0 .. n-1)
// to the row sums of the stage cost's pattern: d = sum_j (o^p_j - o^0_j)^2, fmaf over the columns j = rc, rc + 8, ..,
// then the butterfly over the row's 8 lanes.  xs advances by the nominal output alone, with the operations of the
// plain rollout.  Returns d of row rrow (the same in its 8 lanes); the operand block is free on return.
template <bool BF16, typename Ens>
__device__ __forceinline__ float cem_disagree_step(const MlpDesc& dyn, const Ens& ens, uint32_t mem, int n, float* Ab,
                                                   __bf16* Hb, DgTiles& xs, int wave, int lane, int rrow, int rc) {
  const int l16 = lane & 15, L = dyn.L;
  const CemNominal& nom = ens.nominal();
  auto prod = [&](int l, const float* W, DgTiles& out) {
    const int K = dyn.dims[l], Nl = dyn.dims[l + 1];
    if constexpr (BF16)
      dg_gemm_bf16(Hb, dg_kp(K), dg_np(Nl), reinterpret_cast<const __bf16*>(W), wave, lane, out);
    else
      dg_gemm(Ab, K, Nl, W, wave, lane, out);
  };
  auto hidden = [&](int l, const DgTiles& v, const float* bias) {
    const int Nl = dyn.dims[l + 1];
    auto act = [bias](float x, int j) { return fmaxf(x + bias[j], 0.f); };
    if constexpr (BF16)
      cem_store_tiles16<false, true>(Ab, Hb, v, Nl, dg_kp(Nl), wave, lane, act);
    else
      cem_store_tiles(Ab, v, Nl, wave, lane, act);
  };
  // acc: the running layer's product.  om: first the nominal network's layer-0 product, taken beside the member's
  // while the input stands; at the end of the member's pass the two change places -- acc the nominal product, om = o^p
  DgTiles acc, om;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass)
    for (int l = 0; l < L; ++l) {
      const float* bias = pass ? nom.b[l] : ens.b(dyn.b[l], mem);
      if (pass == 0 || l > 0) {
        prod(l, pass ? nom.W[l] : ens.W(dyn.W[l], mem), acc);
        if (pass == 0 && l == 0) prod(0, nom.W[0], om);
        __syncthreads();   // every wave has read its operand rows (at layer 0: and the stage cost its row)
      }
      if (l < L - 1) {
        hidden(l, acc, bias);
        __syncthreads();
        continue;
      }
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) {
        const int j = (wave + 4 * ci) * 16 + l16;
        const float bj = j < n ? bias[j] : 0.f;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const float op = acc.p[ci][rr] + bj, oq = acc.q[ci][rr] + bj;     // this pass's output
          if (pass == 0) {
            acc.p[ci][rr] = om.p[ci][rr];
            acc.q[ci][rr] = om.q[ci][rr];
            om.p[ci][rr] = op;
            om.q[ci][rr] = oq;
          } else if (j < n) {
            om.p[ci][rr] = om.p[ci][rr] - op;
            om.q[ci][rr] = om.q[ci][rr] - oq;
            xs.p[ci][rr] = op + xs.p[ci][rr];
            xs.q[ci][rr] = oq + xs.q[ci][rr];
          }
        }
      }
    }
  cem_store_tiles(Ab, om, n, wave, lane, [](float v, int) { return v; });
  __syncthreads();
  const float* row = Ab + rrow * GMPC_DG_LDA;
  float sd = 0.f;
  for (int j = rc; j < n; j += 8) sd = fmaf(row[j], row[j], sd);
  sd = cem_row8_sum(sd);
  __syncthreads();   // the rows are read: the next step's input may be stored
  return sd;
}

template <bool BF16, typename Src, typename Ens = CemOneModel>
__device__ __forceinline__ void cem_rollout_body(const CemRollArgs& a, int rows, int ldc, float* Ab, __bf16* Hb,
                                                 Src& src, const Ens& ens = Ens()) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, kq = lane >> 4;
  const int n = a.n, m = a.m, T = a.T;
  const int tiles = (rows + GMPC_CEM_ROWS - 1) / GMPC_CEM_ROWS;
  const int b = blockIdx.x / tiles, s0 = (blockIdx.x - b * tiles) * GMPC_CEM_ROWS;
  const int rrow = tid >> 3, rc = tid & 7;   // the row whose sums this thread shares in, its lane of the row's 8
  const float w0 = sigmoidf_(a.mpc_w[0]), w1 = sigmoidf_(a.mpc_w[1]), w2 = sigmoidf_(a.mpc_w[2]);
  const float al = GMPC_ALPHA;
  src.begin(b, s0, tid);
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
  [[maybe_unused]] float dsum = 0.f;   // CemDisagree: the disagreement D of row rrow so far
  DgTiles acc;
  for (int t = 0; t < T; ++t) {
    const uint32_t mem = ens.step(t);     // the member this step runs under (CemParticle; 0 and unused otherwise)
    // ---- layer 0 input [x_t; u_t]
    if constexpr (BF16) {
      cem_store_tiles16<true, true>(Ab, Hb, xs, n, n, wave, lane, [](float v, int) { return v; });
      const int w = dg_kp(n + m) - n;     // the controls' columns and the zeros behind them
      for (int e = tid; e < GMPC_CEM_ROWS * w; e += GMPC_DG_THREADS) {
        const int i = e / w, j = e - i * w, s = s0 + i;
        float u = 0.f;
        if (j < m) {
          u = src.control(b, i, s, t, j);
          Ab[i * GMPC_DG_LDA + n + j] = u;
          if (ens.records()) src.record(b, s, t, j, u);
        }
        Hb[i * GMPC_DG_LDH + n + j] = static_cast<__bf16>(u);
      }
    } else {
      cem_store_tiles(Ab, xs, n, wave, lane, [](float v, int) { return v; });
      for (int e = tid; e < GMPC_CEM_ROWS * m; e += GMPC_DG_THREADS) {
        const int i = e / m, j = e - i * m, s = s0 + i;
        const float u = src.control(b, i, s, t, j);
        Ab[i * GMPC_DG_LDA + n + j] = u;
        if (ens.records()) src.record(b, s, t, j, u);
      }
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
    // ---- x_{t+1} = x_t + MLP([x_t; u_t]); CemDisagree: the member's pass beside the nominal one, D += d_t
    if constexpr (Ens::disagree)
      dsum += cem_disagree_step<BF16>(a.dyn, ens, mem, n, Ab, Hb, xs, wave, lane, rrow, rc);
    else for (int l = 0; l < a.dyn.L; ++l) {
      const int K = a.dyn.dims[l], Nl = a.dyn.dims[l + 1];
      if constexpr (BF16)
        dg_gemm_bf16(Hb, dg_kp(K), dg_np(Nl), reinterpret_cast<const __bf16*>(ens.W(a.dyn.W[l], mem)), wave, lane,
                     acc);
      else
        dg_gemm(Ab, K, Nl, ens.W(a.dyn.W[l], mem), wave, lane, acc);
      __syncthreads();   // every wave has read its operand rows (and the stage cost its row)
      const float* bias = ens.b(a.dyn.b[l], mem);
      if (l < a.dyn.L - 1) {
        auto act = [bias](float v, int j) { return fmaxf(v + bias[j], 0.f); };
        if constexpr (BF16)
          cem_store_tiles16<false, true>(Ab, Hb, acc, Nl, dg_kp(Nl), wave, lane, act);
        else
          cem_store_tiles(Ab, acc, Nl, wave, lane, act);
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
  if constexpr (BF16)
    cem_store_tiles16<false, true>(Ab, Hb, xs, n, dg_kp(n), wave, lane, [](float v, int) { return v; });
  else
    cem_store_tiles(Ab, xs, n, wave, lane, [](float v, int) { return v; });
  __syncthreads();
  for (int l = 0; l < a.cost.L; ++l) {
    const int K = a.cost.dims[l], Nl = a.cost.dims[l + 1];
    if constexpr (BF16)
      dg_gemm_bf16(Hb, dg_kp(K), dg_np(Nl), reinterpret_cast<const __bf16*>(a.cost.W[l]), wave, lane, acc);
    else
      dg_gemm(Ab, K, Nl, a.cost.W[l], wave, lane, acc);
    __syncthreads();
    const float* bias = a.cost.b[l];
    auto act = [bias](float v, int j) { return fmaxf(v + bias[j], 0.f); };
    auto lin = [bias](float v, int j) { return v + bias[j]; };
    if constexpr (BF16) {
      if (l < a.cost.L - 1)
        cem_store_tiles16<false, true>(Ab, Hb, acc, Nl, dg_kp(Nl), wave, lane, act);
      else
        cem_store_tiles16<true, false>(Ab, Hb, acc, Nl, Nl, wave, lane, lin);     // fp32, unrounded: what |y|^2 reads
    } else {
      if (l < a.cost.L - 1)
        cem_store_tiles(Ab, acc, Nl, wave, lane, act);
      else
        cem_store_tiles(Ab, acc, Nl, wave, lane, lin);
    }
    __syncthreads();
  }
  {
    const float* row = Ab + rrow * GMPC_DG_LDA;
    const int fout = a.cost.dims[a.cost.L];
    float sy = 0.f;
    for (int j = rc; j < fout; j += 8) sy = fmaf(row[j], row[j], sy);
    sy = cem_row8_sum(sy);
    csum += w2 * sy;
    if constexpr (Ens::disagree) csum = cem_penalised(csum, ens.penalty, dsum);
    if (rc == 0 && s0 + rrow < rows) ens.costs(a.costs)[(size_t)b * ldc + s0 + rrow] = csum;
  }
}

// The one kernel of the sampled rollout: the operand block or blocks at the start of the dynamic LDS, the source's own
// LDS behind them, then the body.  Sixteen instantiations, {CemDrawn, IcemDrawn} x {fp32, bf16} x {CemOneModel,
// CemMember, CemParticle, CemDisagree}, explicit in gmpc_cem.hip and gmpc_icem.hip.
template <typename Src, bool BF16, typename Ens>
__global__ __launch_bounds__(GMPC_DG_THREADS) void k_sampled_rollout(typename Src::Args a, Ens e) {
  extern __shared__ __attribute__((aligned(16))) char smem_roll[];
  float* Ab = reinterpret_cast<float*>(smem_roll);   // [32][GMPC_DG_LDA] fp32: the layer inputs of the 32 rows (bf16
                                                     // mode: [x_t; u_t] and the last cost output)
  __bf16* Hb = BF16 ? reinterpret_cast<__bf16*>(smem_roll + GMPC_CEM_LDS32) : nullptr;   // [32][GMPC_DG_LDH]
  Src src(a, smem_roll + (BF16 ? GMPC_CEM_LDS16 : GMPC_CEM_LDS32));
  cem_rollout_body<BF16>(Src::roll(a), Src::rows(a), Src::ldc(a), Ab, Hb, src, e);
}

// Host side.  The launch of one precision: the grid -- tiles of 32 rows per problem by members (TS1: by particles) --
// and, under an ensemble, the reduce of the planes' costs behind it
template <typename Src, bool BF16>
static void sampled_launch_form(const typename Src::Args& a, size_t lds, const CemEnsemble* ens, hipStream_t s) {
  const CemRollArgs& c = Src::roll(a);
  const int rows = Src::rows(a), ldc = Src::ldc(a), tiles = (rows + GMPC_CEM_ROWS - 1) / GMPC_CEM_ROWS;
  const dim3 grid(c.B * tiles, ens ? ens->Q : 1);
  if (!ens) {
    hipLaunchKernelGGL((k_sampled_rollout<Src, BF16, CemOneModel>), grid, dim3(GMPC_DG_THREADS), lds, s, a,
                       CemOneModel());
    return;
  }
  if (ens->disagree) {
    const CemDisagree dg{ens->wstride, ens->bstride, (size_t)c.B * ldc, ens->part, ens->nom, ens->penalty};
    hipLaunchKernelGGL((k_sampled_rollout<Src, BF16, CemDisagree>), grid, dim3(GMPC_DG_THREADS), lds, s, a, dg);
  } else if (ens->ts1) {
    const CemParticle pt{ens->wstride, ens->bstride, (size_t)c.B * ldc, ens->part, (uint32_t)ens->P, c.rng.key0,
                         c.rng.key1, c.rng.it};
    hipLaunchKernelGGL((k_sampled_rollout<Src, BF16, CemParticle>), grid, dim3(GMPC_DG_THREADS), lds, s, a, pt);
  } else {
    const CemMember mb{ens->wstride, ens->bstride, (size_t)c.B * ldc, ens->part};
    hipLaunchKernelGGL((k_sampled_rollout<Src, BF16, CemMember>), grid, dim3(GMPC_DG_THREADS), lds, s, a, mb);
  }
  gmpc_launch_ens_reduce(*ens, c.B, rows, ldc, c.costs, s);
}

// The one launcher.  Non-zero (nothing launched) outside the covered shapes -- widths and n + m up to
// GMPC_SAMPLED_MAX_WIDTH, 1 .. GMPC_CEM_MAX_N rows -- for the mean_row form in anything but fp32 on one model, for X
// under an ensemble, and where the source refuses.  ens: null, or the ensemble whose members all roll the rows out
// (the arguments' dyn: member 0; bf16: its images).
template <typename Src>
static int sampled_launch_rollout(const typename Src::Args& a0, bool bf16, const CemEnsemble* ens, hipStream_t s) {
  typename Src::Args a = a0;
  const CemRollArgs& c = Src::roll(a);
  for (int l = 0; l <= c.dyn.L; ++l)
    if (c.dyn.dims[l] > GMPC_SAMPLED_MAX_WIDTH) return 1;
  for (int l = 0; l <= c.cost.L; ++l)
    if (c.cost.dims[l] > GMPC_SAMPLED_MAX_WIDTH) return 1;
  const int rows = Src::rows(a);
  if (c.n + c.m > GMPC_SAMPLED_MAX_WIDTH || rows < 1 || rows > GMPC_CEM_MAX_N || Src::ldc(a) < rows) return 1;
  if (c.mean_row && (bf16 || ens)) return 1;     // (the returned sequence's rollout is the fp32 kernel's)
  if (ens && (c.X || ens->P < 1 || ens->P > GMPC_MAX_ENSEMBLE || !ens->part)) return 1;
  if (ens && (ens->Q < 1 || ens->Q > GMPC_MAX_ENSEMBLE || (!ens->ts1 && ens->Q != ens->P))) return 1;
  if (ens && ens->disagree && ens->ts1) return 1;
  const size_t blocks = bf16 ? GMPC_CEM_LDS16 : GMPC_CEM_LDS32;
  size_t extra = 0;
  if (Src::plan(a, blocks, &extra)) return 1;
  if (bf16)
    sampled_launch_form<Src, true>(a, blocks + extra, ens, s);
  else
    sampled_launch_form<Src, false>(a, blocks + extra, ens, s);
  return 0;
}

// ---- the keys of the update -----------------------------------------------------------------------------------
// Order-preserving bits of a cost (a NaN sorts as +inf, -0 as +0), then the row index: ascending keys = the stable
// order
__device__ __forceinline__ unsigned long long cem_key(float c, int i) {
  uint32_t u = c != c ? 0x7F800000u : c == 0.f ? 0u : __float_as_uint(c);
  u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
  return ((unsigned long long)u << 32) | (uint32_t)i;
}

// Bitonic sort of keys [P] in LDS by the whole workgroup, P a power of two; the caller has synchronised behind the
// writes of the keys, and every thread may read them on return
__device__ __forceinline__ void cem_sort_keys(unsigned long long* keys, int P, int tid) {
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
}
