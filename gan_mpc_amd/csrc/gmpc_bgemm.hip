// Batched "TN" GEMM family: C[b] = alpha * sum_k X[b][k][0:M]^T (x) Y[b][k][0:N]  (+ beta * C[b]), every operand
// row-major, so row k of X / Y IS the MFMA A / B operand of k-step k and all global reads are coalesced.  Callers:
// the large-state backward pass (gmpc_large.hip), the critic's wide-input route (gmpc_api_critic.hip) and the
// exported gmpc_bgemm_tn.  gmpc_launch_bgemm_tn picks one of three kernels from the shape and the options set in
// BgemmArgs (gmpc_device.h; bgemm_args fills the plain product).  What the callers rely on:
//   - TN form only: X[b] is K x M, Y[b] is K x N, C[b] is M x N; a batch stride of 0 shares an operand; batch elements
//     whose `active` entry is 0 are left untouched.
//   - pad rows and columns of Y: the one-wave strips (k_bgemm_tn) read Y up to 4 rows past K and up to 32*NTW-1 columns
//     past N (values discarded, never multiplied: a NaN there is harmless), so Y[b] + K * ldy is followed by
//     max(8 * ldy, 4 * ldy + 32 * NTW) readable floats: 8 rows, which cover it whenever 4 * ldy >= 32 * NTW.  The
//     streaming kernel (k_bthin) and the LDS-staged one (k_bgemm_tn_lds) clamp / zero-fill at the edges: never
//     outside the matrix.
//   - options that exist in the LDS-staged kernel only: the epilogue addend E, `rowmask` and the further K-segments
//     K2 / K3 -- setting one of them routes the product there whatever its shape -- and `upper_only`, which does NOT
//     route by itself: the streaming kernel is ruled out, but a shape that the strips take (M <= 32 or N <= 64, no
//     other option) gets the full product from them, which is a valid answer.
//   - gmpc_bgemm_route_of is the dispatcher's decision without its launch; gmpc_bgemm_tn_ex / gmpc_bgemm_route
//     (gmpc_api_critic.hip) export the full BgemmArgs and the decision for tests/bgemm_cases.py.
#include <type_traits>

#include "gmpc_launch.h"

// ------------------------------------------------------------------------------------------------
// C[b] = alpha * sum_{k<K} X[b][k][0:M]^T (x) Y[b][k][0:N]  (+ beta * C[b]);  one wave per
// 32 x 32*NTW strip of one batch element.  Y is read up to 4 rows past K and up to 32*NTW-1 columns
// past N (values discarded, never multiplied): the caller pads its buffers.
// ------------------------------------------------------------------------------------------------
template <int NTW>
__global__ __launch_bounds__(GMPC_THREADS) void k_bgemm_tn(BgemmArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const int mstrips = (a.M + 31) >> 5, ngroups = (a.N + 32 * NTW - 1) / (32 * NTW);
  const long total = (long)a.batch * mstrips * ngroups;
  const long item = (long)blockIdx.x * (GMPC_THREADS / 64) + wave;
  if (item >= total) return;
  const int b = (int)(item / (mstrips * ngroups));
  const int rem = (int)(item - (long)b * mstrips * ngroups);
  const int mi = rem / ngroups, ng = rem - mi * ngroups;
  if (a.active != nullptr && a.active[b] == 0) return;
  const float* X = a.X + (size_t)b * a.sx;
  const float* Y = a.Y + (size_t)b * a.sy;
  float* C = a.C + (size_t)b * a.sc;
  const int K = a.K, Kp = K & ~1;
  const int acol = mi * 32 + l31;
  const bool aok = acol < a.M;
  const float* ap = X + (aok ? acol : a.M - 1);
  const int ldx = a.ldx;
  auto afn = [&](int k0) -> float {
    const int r = k0 + half;
    const float v = ap[(size_t)min(r, K - 1) * ldx];
    return (aok && r < K) ? v : 0.f;
  };
  f32x16 acc[NTW];
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) acc[nt][rg] = 0.f;
  const float* bp0 = Y + (size_t)half * a.ldy + ng * 32 * NTW + l31;
  if (Kp > 0) gemm_tile<NTW>(bp0, a.ldy, Kp, afn, acc);
  if (K & 1) {
    // odd K: the last k-step pairs row K-1 with a zero row.  Row K of Y belongs to somebody else
    // (the next batch element or time step) and may hold NaN, which 0 * x would let through.
    const float av = half == 0 ? afn(K - 1) : 0.f;
    const float* yr = Y + (size_t)(K - 1) * a.ldy + ng * 32 * NTW + l31;
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
      const float bv = half == 0 ? yr[nt * 32] : 0.f;
      acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[nt], 0, 0, 0);
    }
  }
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt) {
    const int col = ng * 32 * NTW + nt * 32 + l31;
    if (col < a.N) {
#pragma unroll
      for (int rg = 0; rg < 16; ++rg) {
        const int row = mi * 32 + (rg & 3) + 8 * (rg >> 2) + 4 * half;
        if (row < a.M) {
          float* cp = C + (size_t)row * a.ldc + col;
          float v = a.alpha * acc[nt][rg];
          if (a.beta != 0.f) v = fmaf(a.beta, *cp, v);
          *cp = v;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Streaming form of the thin products (k_bthin<WIDE_X>): one operand has at most 32 columns per strip, the
// other one is wide and comes from HBM exactly once per strip (PB = P B and [H | G_r] = B^T [PA | PB] of the
// large-state pass: 290 / 302 MB per time step at the C4 shard).  k_bgemm_tn reads the wide operand one dword
// per lane and k-step with two k-steps in flight: ~1 KB per wave on its way at a time, 1.1-1.7 TB/s.  Here a
// wave owns 128 consecutive columns of the wide operand as FOUR interleaved MFMA tiles -- tile j = columns
// 128 g + 4 i + j, i = 0..31 -- so a lane's 16-byte load of row 2 ks + half IS the operand of the four tiles
// (the matrix instruction does not care which column sits in which tile row as long as the epilogue knows),
// and BT_RD k-steps are in flight (BT_RD KB per wave; 6 or 10 measure the same).  The rows need not be 16-byte aligned (n + m = 393 at
// C4): the loads carry 4-byte alignment, which the memory pipeline of gfx950 serves in its unaligned mode.
// The wide operand is read up to 127 columns past its width in its last column group (clamped to the row's
// last 16 bytes: never out of the matrix), rows past K are not read (clamped, the thin operand is zero there).
// ------------------------------------------------------------------------------------------------
#define BT_RD 10
struct __attribute__((packed, aligned(4))) bt_f4 { float x, y, z, w; };
struct __attribute__((packed, aligned(4))) bt_f2 { float x, y; };

// NTJ = 2: 64 columns per wave, 8-byte loads (twice the waves: fills the chip when batch * width / 128 does not)
// NS = 2: both 32-column strips of a thin operand of 33..64 columns in one wave (the wide operand is read once)
template <bool WIDE_X, int NTJ, int RD, int NS>
__global__ __launch_bounds__(GMPC_THREADS) void k_bthin(BgemmArgs a) {
  constexpr int GW = 32 * NTJ;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const int Wd = WIDE_X ? a.M : a.N, Th = WIDE_X ? a.N : a.M;       // wide / thin extents
  const int groups = (Wd + GW - 1) / GW, strips = (Th + 32 * NS - 1) / (32 * NS);
  const long total = (long)a.batch * groups * strips;
  const long item = (long)blockIdx.x * (GMPC_THREADS / 64) + wave;
  if (item >= total) return;
  const int b = (int)(item / (groups * strips));
  const int rem = (int)(item - (long)b * groups * strips);
  const int g = rem / strips, st = rem - g * strips;
  if (a.active != nullptr && a.active[b] == 0) return;
  const float* Wp = (WIDE_X ? a.X + (size_t)b * a.sx : a.Y + (size_t)b * a.sy);
  const float* Tp = (WIDE_X ? a.Y + (size_t)b * a.sy : a.X + (size_t)b * a.sx);
  const int ldw = WIDE_X ? a.ldx : a.ldy, ldt = WIDE_X ? a.ldy : a.ldx;
  const int K = a.K;
  // this lane's NTJ wide columns and its thin column(s)
  const int wc = GW * g + NTJ * l31;
  // lanes past the width read the row's last 16 bytes instead (never out of the matrix); when the width is not
  // a multiple of 4 one lane straddles the edge and finds its columns `sh` places further up in that load
  const int wcl = min(wc, max(Wd - NTJ, 0));
  const int sh = wc - wcl;
  const bool ragged = (Wd & (NTJ - 1)) != 0;        // (uniform)
  const int tc0 = 32 * NS * st + l31;
  const float* wrow = Wp + wcl;
  const float* trow[NS];
  bool tok[NS];
#pragma unroll
  for (int q = 0; q < NS; ++q) {
    tok[q] = tc0 + 32 * q < Th;
    trow[q] = Tp + (tok[q] ? tc0 + 32 * q : 0);
  }
  f32x16 acc[NS][NTJ];
#pragma unroll
  for (int q = 0; q < NS; ++q)
#pragma unroll
    for (int j = 0; j < NTJ; ++j)
#pragma unroll
      for (int rg = 0; rg < 16; ++rg) acc[q][j][rg] = 0.f;
  struct Tq { float v[NS]; };
  bt_f4 wq[RD];
  Tq tq[RD];
  const int KS = (K + 1) >> 1;
  auto issue = [&](int ks, bt_f4& wv, Tq& tv) {
    const int r = min(2 * ks + half, K - 1);
    if (NTJ == 4) {
      wv = *reinterpret_cast<const bt_f4*>(wrow + (size_t)r * ldw);
    } else {
      const bt_f2 q = *reinterpret_cast<const bt_f2*>(wrow + (size_t)r * ldw);
      wv.x = q.x; wv.y = q.y;
    }
#pragma unroll
    for (int q = 0; q < NS; ++q) tv.v[q] = trow[q][(size_t)r * ldt];
  };
  auto mult = [&](int ks, bt_f4 wv, const Tq& tv) {
    const bool rok = 2 * ks + half < K;
    if (ragged) {
      const bt_f4 q = wv;
      if (NTJ == 4) {
        wv.x = sh == 0 ? q.x : sh == 1 ? q.y : sh == 2 ? q.z : q.w;
        wv.y = sh == 0 ? q.y : sh == 1 ? q.z : q.w;
        wv.z = sh == 0 ? q.z : q.w;
      } else {
        wv.x = sh == 0 ? q.x : q.y;
      }
    }
    const float wj[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
    for (int q = 0; q < NS; ++q) {
      const float t = (tok[q] && rok) ? tv.v[q] : 0.f;
#pragma unroll
      for (int j = 0; j < NTJ; ++j)
        acc[q][j] = WIDE_X ? __builtin_amdgcn_mfma_f32_32x32x2f32(wj[j], t, acc[q][j], 0, 0, 0)
                           : __builtin_amdgcn_mfma_f32_32x32x2f32(t, wj[j], acc[q][j], 0, 0, 0);
    }
  };
#pragma unroll
  for (int i = 0; i < RD; ++i) issue(min(i, KS - 1), wq[i], tq[i]);
  int ks = 0;
  for (; ks + RD <= KS; ks += RD) {
#pragma unroll
    for (int i = 0; i < RD; ++i) {
      const bt_f4 wv = wq[i];
      const Tq tv = tq[i];
      issue(min(ks + RD + i, KS - 1), wq[i], tq[i]);      // (past the end: the last k-step again, not used)
      __builtin_amdgcn_sched_barrier(0);
      mult(ks + i, wv, tv);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int i = 0; i < RD; ++i)
    if (ks + i < KS) mult(ks + i, wq[i], tq[i]);
  // epilogue: accumulator row i of tile j <-> wide column GW g + NTJ i + j (WIDE_X: a row of C), column l31 <->
  // thin column (WIDE_X) / wide columns GW g + NTJ l31 + j (a run of NTJ floats of row i of C otherwise)
#pragma unroll
  for (int q = 0; q < NS; ++q) {
    const int tc = tc0 + 32 * q;
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) {
      const int i = (rg & 3) + 8 * (rg >> 2) + 4 * half;
      if (WIDE_X) {
#pragma unroll
        for (int j = 0; j < NTJ; ++j) {
          const int row = GW * g + NTJ * i + j;
          if (row < a.M && tok[q]) {
            float* cp = a.C + (size_t)b * a.sc + (size_t)row * a.ldc + tc;
            float v = a.alpha * acc[q][j][rg];
            if (a.beta != 0.f) v = fmaf(a.beta, *cp, v);
            *cp = v;
          }
        }
      } else {
        const int row = 32 * NS * st + 32 * q + i;
        if (row < a.M) {
          float* cp = a.C + (size_t)b * a.sc + (size_t)row * a.ldc + wc;
          if (wc + NTJ <= a.N) {             // the lane's NTJ columns as one store (a row of C is contiguous)
            float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < NTJ; ++j) v[j] = a.alpha * acc[q][j][rg];
            if (NTJ == 4) {
              bt_f4* c4 = reinterpret_cast<bt_f4*>(cp);
              if (a.beta != 0.f) {
                const bt_f4 o = *c4;
                v[0] = fmaf(a.beta, o.x, v[0]); v[1] = fmaf(a.beta, o.y, v[1]);
                v[2] = fmaf(a.beta, o.z, v[2]); v[3] = fmaf(a.beta, o.w, v[3]);
              }
              *c4 = bt_f4{v[0], v[1], v[2], v[3]};
            } else {
              bt_f2* c2 = reinterpret_cast<bt_f2*>(cp);
              if (a.beta != 0.f) {
                const bt_f2 o = *c2;
                v[0] = fmaf(a.beta, o.x, v[0]); v[1] = fmaf(a.beta, o.y, v[1]);
              }
              *c2 = bt_f2{v[0], v[1]};
            }
          } else {
#pragma unroll
            for (int j = 0; j < NTJ; ++j) {
              if (wc + j < a.N) {
                float v = a.alpha * acc[q][j][rg];
                if (a.beta != 0.f) v = fmaf(a.beta, cp[j], v);
                cp[j] = v;
              }
            }
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// LDS-tiled variant for products whose M and N are both large: a workgroup of 4 waves (2 x 2) owns a
// (64*WMT) x (64*WNT) block of C[b]; KC rows of X and Y at a time are staged through LDS (double
// buffered, zero-filled past the matrix edges, so nothing is read out of bounds and a NaN in a
// neighbouring matrix cannot leak in), each wave runs WMT x WNT MFMA tiles per k-step from it.
// Against one-wave strips this cuts the L2 traffic per output ~3x, which is what bounded them.
// A second K-segment (X2, Y2, K2) is accumulated into the same tile.
// ------------------------------------------------------------------------------------------------
// VEC: operands whose leading dimensions, sizes and base addresses are multiples of 4 floats are staged
// with 16-byte loads and LDS writes (a quarter of the staging instructions).
template <int WMT, int WNT, int KC, bool VEC = false>
__global__ __launch_bounds__(GMPC_THREADS, 2) void k_bgemm_tn_lds(BgemmArgs a) {
  constexpr int BM = 64 * WMT, BN = 64 * WNT;
  constexpr int VW = VEC ? 4 : 1;
  constexpr int LX = KC * BM / GMPC_THREADS / VW, LY = KC * BN / GMPC_THREADS / VW;
  static_assert(!VEC || ((KC * BM) % (4 * GMPC_THREADS) == 0 && (KC * BN) % (4 * GMPC_THREADS) == 0), "vec staging");
  typedef typename std::conditional<VEC, float4, float>::type stage_t;
  __shared__ __attribute__((aligned(16))) float Xs[2][KC][BM];
  __shared__ __attribute__((aligned(16))) float Ys[2][KC][BN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const int wm = wave >> 1, wn = wave & 1;
  const int mb = (a.M + BM - 1) / BM, nb = (a.N + BN - 1) / BN;
  // upper-only outputs: the grid holds the LIVE blocks only (row block mi keeps column blocks ni >= mi BM / BN: the
  // ones with an element on or above the diagonal), `a.upper_only` = their number per batch element.  (With the dead
  // blocks in the grid as workgroups that return at once, a 128 x 256 tiling of T1 took the time of the full product.)
  const int lb = a.upper_only ? a.upper_only : mb * nb;
  const long total = (long)a.batch * lb;
  // consecutive workgroup ids go round the 8 XCDs: give every XCD one contiguous range of blocks,
  // so the blocks sharing a batch element's X / Y panels meet in the same L2
  const long per = (total + 7) / 8;
  const long item = (long)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
  if ((long)(blockIdx.x >> 3) >= per || item >= total) return;
  const int b = (int)(item / lb);
  int rem = (int)(item - (long)b * lb);
  int mi, ni;
  if (a.upper_only) {
    mi = 0;
    int live = nb;                                   // live blocks of row block mi
    while (rem >= live) { rem -= live; ++mi; live = nb - (mi * BM) / BN; }
    ni = (mi * BM) / BN + rem;
  } else {
    mi = rem / nb;
    ni = rem - mi * nb;
  }
  if (a.active != nullptr && a.active[b] == 0) return;
  const int m0 = mi * BM, n0 = ni * BN;
  // ... and in a block on the diagonal the wave whose 32 WMT x 32 WNT corner lies below it (one of four in a
  // square block) only helps with the staging: no MFMAs, no stores
  const bool dead = a.upper_only && m0 + wm * WMT * 32 > n0 + (wn * WNT + WNT) * 32 - 1;
  f32x16 acc[WMT][WNT];
#pragma unroll
  for (int i = 0; i < WMT; ++i)
#pragma unroll
    for (int j = 0; j < WNT; ++j)
#pragma unroll
      for (int rg = 0; rg < 16; ++rg) acc[i][j][rg] = 0.f;
  stage_t rxx[2][LX], ryy[2][LY];   // chunk c travels in set c & 1: two chunks of loads in flight
  const int c1 = (a.K + KC - 1) / KC, c2 = (a.K2 + KC - 1) / KC, c3 = (a.K3 + KC - 1) / KC, nc = c1 + c2 + c3;
  auto zero = []() { stage_t z; memset(&z, 0, sizeof(z)); return z; };
  // Full chunks (all KC rows inside K) are staged through buffer resources: the chunk's row offset is an
  // SGPR, each thread's element offset a loop-invariant VGPR, and a column past the edge is an offset
  // past the resource (the load returns 0) -- no address arithmetic or predicates between the MFMAs
  // (they were ~50 VALU instructions per 32 MFMAs; with two waves per SIMD each costs matrix-pipe time).
  constexpr unsigned OOB = 0x7ff00000u;     // beyond any operand of one batch element (< 2 GB each)
  const __amdgpu_buffer_rsrc_t rX1 = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.X + (size_t)b * a.sx), 0, (int)(((size_t)(a.K - 1) * a.ldx + a.M) * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rY1 = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(a.Y + (size_t)b * a.sy), 0, (int)(((size_t)(a.K - 1) * a.ldy + a.N) * 4), 0x00020000);
  const bool seg2 = a.K2 > 0;
  const __amdgpu_buffer_rsrc_t rX2 = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(seg2 ? a.X2 + (size_t)b * a.sx2 : a.X), 0,
      seg2 ? (int)(((size_t)(a.K2 - 1) * a.ldx2 + a.M) * 4) : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rY2 = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(seg2 ? a.Y2 + (size_t)b * a.sy2 : a.Y), 0,
      seg2 ? (int)(((size_t)(a.K2 - 1) * a.ldy2 + a.N) * 4) : 0, 0x00020000);
  const bool seg3 = a.K3 > 0;
  const __amdgpu_buffer_rsrc_t rX3 = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(seg3 ? a.X3 + (size_t)b * a.sx3 : a.X), 0,
      seg3 ? (int)(((size_t)(a.K3 - 1) * a.ldx3 + a.M) * 4) : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rY3 = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(seg3 ? a.Y3 + (size_t)b * a.sy3 : a.Y), 0,
      seg3 ? (int)(((size_t)(a.K3 - 1) * a.ldy3 + a.N) * 4) : 0, 0x00020000);
  unsigned vx1[LX], vx2[LX], vx3[LX], vy1[LY], vy2[LY], vy3[LY];
#pragma unroll
  for (int j = 0; j < LX; ++j) {
    const int e = (tid + GMPC_THREADS * j) * VW, r = e / BM, c = e % BM;
    const bool ok = m0 + c < a.M;
    vx1[j] = ok ? (unsigned)(((size_t)r * a.ldx + m0 + c) * 4) : OOB;
    vx2[j] = ok ? (unsigned)(((size_t)r * a.ldx2 + m0 + c) * 4) : OOB;
    vx3[j] = ok ? (unsigned)(((size_t)r * a.ldx3 + m0 + c) * 4) : OOB;
  }
#pragma unroll
  for (int j = 0; j < LY; ++j) {
    const int e = (tid + GMPC_THREADS * j) * VW, r = e / BN, c = e % BN;
    const bool ok = n0 + c < a.N;
    vy1[j] = ok ? (unsigned)(((size_t)r * a.ldy + n0 + c) * 4) : OOB;
    vy2[j] = ok ? (unsigned)(((size_t)r * a.ldy2 + n0 + c) * 4) : OOB;
    vy3[j] = ok ? (unsigned)(((size_t)r * a.ldy3 + n0 + c) * 4) : OOB;
  }
  auto bload = [&](const __amdgpu_buffer_rsrc_t& rs, unsigned voff, unsigned soff) -> stage_t {
    stage_t out;
    if constexpr (VEC) {
      typedef unsigned v4u_t __attribute__((ext_vector_type(4)));
      const v4u_t q = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0);
      memcpy(&out, &q, sizeof(out));
    } else {
      const unsigned q = __builtin_amdgcn_raw_buffer_load_b32(rs, voff, soff, 0);
      memcpy(&out, &q, sizeof(out));
    }
    return out;
  };
  auto issue = [&](int ci, stage_t (&rx)[LX], stage_t (&ry)[LY]) {
    const int sg = ci < c1 ? 0 : ci < c1 + c2 ? 1 : 2;       // the K-segment of this chunk
    const int K = sg == 0 ? a.K : sg == 1 ? a.K2 : a.K3;
    const int k0 = (sg == 0 ? ci : sg == 1 ? ci - c1 : ci - c1 - c2) * KC;
    const int ldx = sg == 0 ? a.ldx : sg == 1 ? a.ldx2 : a.ldx3, ldy = sg == 0 ? a.ldy : sg == 1 ? a.ldy2 : a.ldy3;
    // (a chunk that runs past row K - 1 needs no other path: those rows lie beyond the buffer resources, whose
    // loads return 0)
    if ((size_t)(K + KC) * (ldx > ldy ? ldx : ldy) * 4 < OOB) {
      // A full chunk lies inside the resource whatever the range check looks at, so its row offset may ride in
      // the scalar offset (no VALU address arithmetic between the MFMAs).  The chunk that runs past row K - 1
      // RELIES on the range check: there the whole byte offset goes into the per-lane part, which the check is
      // documented to cover -- the scalar offset is not (it is covered on gfx950, which is how the first version
      // of this path passed its tests; nothing here depends on that any more).
      const bool tail = k0 + KC > K;         // wave-uniform
      const unsigned ox = (unsigned)k0 * (unsigned)ldx * 4u, oy = (unsigned)k0 * (unsigned)ldy * 4u;
      const unsigned sx_ = tail ? 0u : ox, sy_ = tail ? 0u : oy, ax = tail ? ox : 0u, ay = tail ? oy : 0u;
      if (sg == 0) {
#pragma unroll
        for (int j = 0; j < LX; ++j) rx[j] = bload(rX1, vx1[j] + ax, sx_);
#pragma unroll
        for (int j = 0; j < LY; ++j) ry[j] = bload(rY1, vy1[j] + ay, sy_);
      } else if (sg == 1) {
#pragma unroll
        for (int j = 0; j < LX; ++j) rx[j] = bload(rX2, vx2[j] + ax, sx_);
#pragma unroll
        for (int j = 0; j < LY; ++j) ry[j] = bload(rY2, vy2[j] + ay, sy_);
      } else {
#pragma unroll
        for (int j = 0; j < LX; ++j) rx[j] = bload(rX3, vx3[j] + ax, sx_);
#pragma unroll
        for (int j = 0; j < LY; ++j) ry[j] = bload(rY3, vy3[j] + ay, sy_);
      }
      return;
    }
    const float* X = sg == 0 ? a.X + (size_t)b * a.sx : sg == 1 ? a.X2 + (size_t)b * a.sx2 : a.X3 + (size_t)b * a.sx3;
    const float* Y = sg == 0 ? a.Y + (size_t)b * a.sy : sg == 1 ? a.Y2 + (size_t)b * a.sy2 : a.Y3 + (size_t)b * a.sy3;
#pragma unroll
    for (int j = 0; j < LX; ++j) {
      const int e = (tid + GMPC_THREADS * j) * VW, r = e / BM, c = e % BM;
      const bool ok = (k0 + r < K) && (m0 + c < a.M);     // VEC: M % 4 == 0, so a group is in or out
      rx[j] = ok ? *reinterpret_cast<const stage_t*>(X + (size_t)(k0 + r) * ldx + m0 + c) : zero();
    }
#pragma unroll
    for (int j = 0; j < LY; ++j) {
      const int e = (tid + GMPC_THREADS * j) * VW, r = e / BN, c = e % BN;
      const bool ok = (k0 + r < K) && (n0 + c < a.N);
      ry[j] = ok ? *reinterpret_cast<const stage_t*>(Y + (size_t)(k0 + r) * ldy + n0 + c) : zero();
    }
  };
  auto stage = [&](int buf, const stage_t (&rx)[LX], const stage_t (&ry)[LY]) {
#pragma unroll
    for (int j = 0; j < LX; ++j) {
      const int e = (tid + GMPC_THREADS * j) * VW;
      *reinterpret_cast<stage_t*>(&Xs[buf][e / BM][e % BM]) = rx[j];
    }
#pragma unroll
    for (int j = 0; j < LY; ++j) {
      const int e = (tid + GMPC_THREADS * j) * VW;
      *reinterpret_cast<stage_t*>(&Ys[buf][e / BN][e % BN]) = ry[j];
    }
  };
  // the loads of chunk c + 2 are issued while chunk c multiplies and chunk c + 1 waits in its registers for
  // the LDS buffer (with one chunk in flight the stage at the end of a chunk waited for loads issued 1.5 k
  // matrix cycles earlier: P and [A | B] come from HBM at the large shapes)
  issue(0, rxx[0], ryy[0]);
  stage(0, rxx[0], ryy[0]);
  if (nc > 1) issue(1, rxx[1], ryy[1]);
  __syncthreads();
  // (the dead wave's chunk is a separate copy: a branch around the MFMAs inside the live one would split the basic
  // block in which the compiler interleaves them with the loads and the LDS writes -- PA at the C4 shard 0.534 ->
  // 0.564 ms)
  auto chunk = [&](int ci, auto par, auto deadc) __attribute__((always_inline)) {
    constexpr int p = decltype(par)::value;            // ci & 1
    constexpr bool DEAD = decltype(deadc)::value;
    const int buf = p;
    if (ci + 2 < nc) issue(ci + 2, rxx[p], ryy[p]);
    if constexpr (!DEAD)
#pragma unroll
    for (int kk = 0; kk < KC; kk += 2) {
      float av[WMT], bv[WNT];
#pragma unroll
      for (int i = 0; i < WMT; ++i) av[i] = Xs[buf][kk + half][(wm * WMT + i) * 32 + l31];
#pragma unroll
      for (int j = 0; j < WNT; ++j) bv[j] = Ys[buf][kk + half][(wn * WNT + j) * 32 + l31];
#pragma unroll
      for (int i = 0; i < WMT; ++i)
#pragma unroll
        for (int j = 0; j < WNT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
    if (ci + 1 < nc) stage(buf ^ 1, rxx[p ^ 1], ryy[p ^ 1]);
    __syncthreads();
  };
  if (dead) {
    for (int ci = 0; ci < nc; ci += 2) {
      chunk(ci, std::integral_constant<int, 0>{}, std::true_type{});
      if (ci + 1 < nc) chunk(ci + 1, std::integral_constant<int, 1>{}, std::true_type{});
    }
    return;
  }
  for (int ci = 0; ci < nc; ci += 2) {
    chunk(ci, std::integral_constant<int, 0>{}, std::false_type{});
    if (ci + 1 < nc) chunk(ci + 1, std::integral_constant<int, 1>{}, std::false_type{});
  }
  float* C = a.C + (size_t)b * a.sc;
#pragma unroll
  for (int i = 0; i < WMT; ++i)
#pragma unroll
    for (int j = 0; j < WNT; ++j) {
      const int col = n0 + (wn * WNT + j) * 32 + l31;
      if (col < a.N) {
        // the addend of the whole tile is requested before the first store (E may alias C as far as the
        // compiler knows: interleaved, every load would wait behind the stores before it).  (All tiles of the
        // wave at once -- one memory round trip per block instead of four -- measured slower: C5 2.059 vs 2.025 s.)
        float ev[16];
        const bool has_e = a.E != nullptr && col < a.En;
#pragma unroll
        for (int rg = 0; rg < 16; ++rg) {
          const int row = m0 + (wm * WMT + i) * 32 + (rg & 3) + 8 * (rg >> 2) + 4 * half;
          ev[rg] = (has_e && row < a.M) ? a.E[(size_t)b * a.se + (size_t)row * a.lde + col] : 0.f;
        }
#pragma unroll
        for (int rg = 0; rg < 16; ++rg) {
          const int row = m0 + (wm * WMT + i) * 32 + (rg & 3) + 8 * (rg >> 2) + 4 * half;
          if (row < a.M) {
            float* cp = C + (size_t)row * a.ldc + col;
            float v = a.alpha * acc[i][j][rg];
            if (a.beta != 0.f) v = fmaf(a.beta, *cp, v);
            v += ev[rg];
            if (a.rowmask != nullptr && !((a.rowmask[(size_t)b * a.srm + (row >> 5)] >> (row & 31)) & 1u)) v = 0.f;
            *cp = v;
          }
        }
      }
    }
}

// rows of X and Y per LDS stage: 16 with 16-byte staging (half the barriers per MFMA; C5 5.95 -> 5.85 s),
// 8 with dword staging (16 there doubles the staging instructions: C4 115 -> 120 ms)
#ifndef GMPC_BG_KC_VEC
#define GMPC_BG_KC_VEC 16
#endif
#ifndef GMPC_BG_KC_VEC22            // stage depth of the 128 x 128 blocks with 16-byte staging (C5: 2.025 s with 8, 2.044 with 16, 2.161 with 32)
#define GMPC_BG_KC_VEC22 8
#endif
#ifndef GMPC_BG_KC
#define GMPC_BG_KC 8
#endif
// The 16-byte staging form and its stage depth follow from the block width and the shape (gmpc_bgemm_route_of below).
template <int WNT, int KC, bool VEC>
static void launch_lds(const BgemmArgs& a0, hipStream_t s) {
  constexpr int BM = 128, BN = 64 * WNT;
  BgemmArgs a = a0;
  const int mbk = (a.M + BM - 1) / BM, nbk = (a.N + BN - 1) / BN;
  long lb = (long)mbk * nbk;
  if (a.upper_only) {                 // live blocks per batch element (see the kernel)
    lb = 0;
    for (int mi = 0; mi < mbk; ++mi) lb += nbk - (mi * BM) / BN > 0 ? nbk - (mi * BM) / BN : 0;
    a.upper_only = (int)lb;
  }
  const long total = (long)a.batch * lb;
  const long per = (total + 7) / 8;
  hipLaunchKernelGGL((k_bgemm_tn_lds<2, WNT, KC, VEC>), dim3((unsigned)(per * 8)), dim3(GMPC_THREADS), 0, s, a);
}

// The dispatcher's decision, apart from its launch (host only, no GPU work: gmpc_bgemm_route exports it so that a test
// can tell which instantiation a shape reaches).
BgemmRoute gmpc_bgemm_route_of(const BgemmArgs& a) {
  // a thin product whose wide operand is worth streaming (k_bthin)
  {
    const bool widex = a.N <= 64 && a.M >= 128, widey = a.M <= 64 && a.N >= 128;
    if ((widex || widey) && a.K >= 2 * BT_RD && a.E == nullptr && a.rowmask == nullptr && a.K2 == 0 &&
        a.K3 == 0 && !a.upper_only) {
      const int Wd = widex ? a.M : a.N, Th = widex ? a.N : a.M;
      // 128 columns per wave (16-byte loads) when that still gives every SIMD a few waves, else 64 (8-byte loads,
      // twice the waves: PB at the C4 shard is 1536 waves of 128 columns -- 1.5 per SIMD, 0.084 ms -- or 3072 of
      // 64, 0.073 ms); a thin operand of 33..64 columns goes through one wave as two strips
      const int ns = Th > 32 ? 2 : 1;
      const long waves4 = (long)a.batch * ((Wd + 127) / 128) * ((Th + 32 * ns - 1) / (32 * ns));
      // (two strips x four tiles are 268 registers, one wave per SIMD: 0.387 ms against 0.360 with two tiles for
      // the [64 x 1088] x K = 200 products of C5)
      const int ntj = (waves4 < 4096 || ns == 2) ? 2 : 4;
      return BgemmRoute{BGEMM_THIN, {widex ? 1 : 0, ntj, ns}};
    }
  }
  // (the epilogue extras and the further K-segments exist in the LDS-staged kernel only)
  if ((a.M > 32 && a.N > 64) || a.E != nullptr || a.rowmask != nullptr || a.K2 > 0 || a.K3 > 0) {
    // column blocks of 128 / 192 / 256: the one that pads N least (ties: the widest)
    // (upper-only outputs: the area of the blocks that are not skipped -- narrow blocks follow the diagonal)
    int best = 2;
    long waste = -1;
    for (int w = 2; w <= 4; ++w) {
      const int bn = 64 * w, nbk = (a.N + bn - 1) / bn;
      long padded = (long)nbk * bn;
      if (a.upper_only) {
        padded = 0;
        for (int mi = 0; mi * 128 < a.M; ++mi)
          for (int ni = 0; ni < nbk; ++ni)
            if (!(mi * 128 > ni * bn + bn - 1)) padded += bn;
      }
      if (waste < 0 || padded <= waste) { waste = padded; best = w; }
    }
    // 16-byte staging needs columns in groups of four (M, N multiples of 4); the ROWS need not start on 16 bytes:
    // buffer_load_dwordx4 takes any 4-byte-aligned address (ld = n + m = 393 at C4)
    // (192-wide blocks stage 16 bytes per thread with 16-row stages only: 8 rows x 192 columns are 1.5 loads per thread)
    const bool vec = (a.M & 3) == 0 && (a.N & 3) == 0;
    return BgemmRoute{BGEMM_LDS, {best, vec ? (best == 2 ? GMPC_BG_KC_VEC22 : GMPC_BG_KC_VEC) : GMPC_BG_KC, vec ? 1 : 0}};
  }
  // a thin product: one wave per strip (the further K-segments are not supported here)
  const int tiles = (a.N + 31) / 32;
  const int ntw = tiles >= 8 && tiles % 8 == 0 ? 8 : tiles >= 6 && tiles % 6 == 0 ? 6
                  : tiles >= 4 ? 4 : tiles >= 2 ? 2 : 1;
  return BgemmRoute{BGEMM_STRIPS, {ntw, 0, 0}};
}

void gmpc_launch_bgemm_tn(const BgemmArgs& a, hipStream_t s) {
  const BgemmRoute r = gmpc_bgemm_route_of(a);
  if (r.family == BGEMM_THIN) {
    const bool widex = r.p[0] != 0;
    const int ntj = r.p[1], ns = r.p[2];
    const int Wd = widex ? a.M : a.N, Th = widex ? a.N : a.M;
    const long total = (long)a.batch * ((Wd + 32 * ntj - 1) / (32 * ntj)) * ((Th + 32 * ns - 1) / (32 * ns));
    const dim3 grid((unsigned)((total + 3) / 4)), blk(GMPC_THREADS);
#define BT_LAUNCH(WX, NJ, S) hipLaunchKernelGGL((k_bthin<WX, NJ, BT_RD, S>), grid, blk, 0, s, a)
    if (ns == 2)       { if (widex) BT_LAUNCH(true, 2, 2); else BT_LAUNCH(false, 2, 2); }
    else if (ntj == 2) { if (widex) BT_LAUNCH(true, 2, 1); else BT_LAUNCH(false, 2, 1); }
    else               { if (widex) BT_LAUNCH(true, 4, 1); else BT_LAUNCH(false, 4, 1); }
#undef BT_LAUNCH
    return;
  }
  if (r.family == BGEMM_LDS) {
    const bool vec = r.p[2] != 0;
    switch (r.p[0]) {
      case 2:
        if (vec) launch_lds<2, GMPC_BG_KC_VEC22, true>(a, s); else launch_lds<2, GMPC_BG_KC, false>(a, s);
        break;
      case 3:
        if (vec) launch_lds<3, GMPC_BG_KC_VEC, true>(a, s); else launch_lds<3, GMPC_BG_KC, false>(a, s);
        break;
      default:
        if (vec) launch_lds<4, GMPC_BG_KC_VEC, true>(a, s); else launch_lds<4, GMPC_BG_KC, false>(a, s);
        break;
    }
    return;
  }
  const int ntw = r.p[0];
  const int mstrips = (a.M + 31) / 32, ngroups = (a.N + 32 * ntw - 1) / (32 * ntw);
  const long total = (long)a.batch * mstrips * ngroups;
  const dim3 grid((unsigned)((total + 3) / 4)), blk(GMPC_THREADS);
  switch (ntw) {
    case 8: hipLaunchKernelGGL(k_bgemm_tn<8>, grid, blk, 0, s, a); break;
    case 6: hipLaunchKernelGGL(k_bgemm_tn<6>, grid, blk, 0, s, a); break;
    case 4: hipLaunchKernelGGL(k_bgemm_tn<4>, grid, blk, 0, s, a); break;
    case 2: hipLaunchKernelGGL(k_bgemm_tn<2>, grid, blk, 0, s, a); break;
    default: hipLaunchKernelGGL(k_bgemm_tn<1>, grid, blk, 0, s, a); break;
  }
}
