// Dynamics Jacobian chain over each sample's ACTIVE relu units only (gfx950; hidden layers all 200 wide, n + m <= 32).
//
// Same product as k_linearize_regs -- [A_t | B_t] - [I | 0] = W_L^T D_{L-1} W_{L-1}^T ... D_1 W_1^T -- and the same
// bits.  The dense chain contracts over all 200 units of a hidden layer; for an inactive unit the running product
// holds an exact zero there, so its term is fma(w, +-0, c) == c (up to the sign of a zero sum).  Both chains issue
// fp32 MFMAs, which accumulate as an fmaf chain in k order: dropping exactly-zero terms and keeping the order of
// the rest reproduces every output.  Outputs of units the next mask zeroes are computed but never read.
//
// One wave per sample, rows 0..15 of its Jacobian on v_mfma_f32_16x16x4_f32: A = W_l^T (16 output units x 4
// contracted units), B = S (4 contracted units x 16 Jacobian rows), the 4 contracted units of a k-step are four
// consecutive entries of the sample's active list.
//  - rows 16..n-1 (n = 17: one row): group jobs of the same kernel body.  A wave owns a contiguous chunk of samples,
//    and the relu masks of consecutive time steps of a trajectory differ in a few units only (about 5 of 200), so
//    every column of a group job's tiles is row r of ANOTHER sample, up to 16 consecutive ones, and the list of a
//    layer is the union of their active sets (about 115 units for 12 - 13 steps).  A column whose sample has unit u
//    inactive must hold an exact +0 there: its extra terms are then fma(w, 0, c) == c, a subset of the zero terms the
//    dense chain adds anyway.  The kernel computes all 200 outputs of a layer and a union list READS what the
//    one-sample list skipped, so the hand-over selects mask(column's sample, unit) ? acc : +0 (keep_if: once per
//    accumulator element and layer, nothing in the k-loop), and the seed is written into the S tile the same way.
//    A strided sample set (samp_mul, samp_add: no caller today) has no consecutive samples: it keeps the strided
//    split and sends rows 16..n-1 to k_linearize_regs, which takes a row window for them.
//  - active lists: built per layer from the relu words with mbcnt (a prefix count, no scan), stored as 32-bit unit
//    indices in the wave's LDS (no 16-bit extensions on the vector port) and padded with unit 200 -- a zero row of
//    the padded W^T copies and a zero column of the S tile -- so the padded k-steps and the loads that run ahead of
//    the last k-step read zeros, in bounds.
//  - A operands: a packed copy of W_l^T made for this kernel (LinPad::WSP, 1 KB per unit, see k_pack_sparse): the
//    12 full 16-unit tiles are three 16-byte buffer loads per lane and k-step, each lane group reading 256
//    contiguous bytes of its row (4 vector-L1 sectors of 64 B; the lane-interleaved rows of k_linearize_regs need 8
//    for the same operands, and the vector L1 retires about one access per cycle); the tail tile is one 4-byte
//    load, 32 contiguous bytes per row.  The voffset is the list entry << 10 plus a lane constant.  A k-step puts its 13 MFMAs beside three list / B
//    reads and three vector instructions (address of the weight rows, of the tail row and of the B operand), plus
//    one pointer increment per list every three k-steps.  (Structured buffer loads, vindex = list entry with the
//    row stride in the resource, would drop the first two, but measured slower: more vector-L1 accesses for the
//    same bytes.)
//  - accumulators: the first k-step starts the chains from the constant zero and the k-loop runs whole groups of
//    three k-steps before the last one or two, so the 52 accumulator registers stay in place: no zeroing and no
//    copies out of the loop per layer.
//  - tail units 192..199: the dense chain sums them on 4x4x1_16B as an even-k partial plus an odd-k partial.  The
//    13th tile reproduces the split: rows 0..7 read unit 192 + r of the even list entries (odd ones -> zero row),
//    rows 8..15 the same units of the odd ones; the two halves are added once per layer, as there.
//  - S between layers: the accumulators go to a wave-private [16 rows][220] LDS tile, the next layer's B operands
//    are read back at the list entries (four distinct units per read, no bank conflict inside a lane group).
#include <cstdio>
#include <type_traits>
#include <utility>

#include "gmpc_launch.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));

#define GMPC_LIN_PADROWS 24  // zero rows behind every padded copy (gmpc_linearize_mfma.hip)
#define GMPC_SP_H 200        // hidden width of this form
#define GMPC_SP_Z 200        // the zero unit padded list entries point at
#define GMPC_SP_STR 220      // floats per Jacobian row of the S tile: units 0..199, zeros 200..207, odd partials 208..215
#define GMPC_SP_CAP 216      // list entries: 200 + the 3 k-steps the prefetch runs ahead, rounded to 8
#define GMPC_SP_WAVE_BYTES (16 * GMPC_SP_STR * 4 + 3 * GMPC_SP_CAP * 4)
#define GMPC_SP_RD 3         // operand sets in flight: loads for k-step p + 2, list entries for p + 3
#define GMPC_SP_ROW 256      // floats per row of a packed copy (1 KB: the row address is the unit << 10)

// The shapes this form covers: two or more hidden layers, all 200 wide, n + m <= 32 (one 32-wide input tile).
static bool sparse_form(int L, const int* dims, int n, int m) {
  const int Lh = L - 1;
  if (Lh < 2 || n + m > 32 || n < 1) return false;
  for (int l = 1; l <= Lh; ++l)
    if (dims[l] != GMPC_SP_H) return false;
  return true;
}

// Packed copy of hidden layer l's W_l^T (W: (200 x 200) row-major, [input unit i][output unit o]).  Row o (a unit of
// layer l + 1, the contracted index) holds the A operands of its k-step as the lanes read them:
//   [64 q + 4 l16 + j] = W[16 (4 q + j) + l16][o]   q = 0..2: tile 4 q + j, unit 16 (4 q + j) + l16 (units 0..191)
//   [192 + u]          = W[192 + u][o]              u = 0..7: the tail tile
// and zeros at 200..255.  Rows 200.. (the zero unit and the padding) stay zero.
__global__ void k_pack_sparse(const float* W, float* dst) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= GMPC_SP_H * GMPC_SP_H) return;
  const int i = e / GMPC_SP_H, o = e - i * GMPC_SP_H;
  const int t = i >> 4;
  const int slot = i < 192 ? 64 * (t >> 2) + 4 * (i & 15) + (t & 3) : i;
  dst[(size_t)o * GMPC_SP_ROW + slot] = W[e];
}

size_t gmpc_linsparse_floats(int L, const int* dims, int n, int m) {
  if (!sparse_form(L, dims, n, m)) return 0;
  // + one row to round the first copy up to 1 KB
  return (size_t)(L - 2) * (GMPC_SP_H + GMPC_LIN_PADROWS) * GMPC_SP_ROW + GMPC_SP_ROW;
}

void gmpc_linsparse_prepare(const MlpDesc& dyn, int n, int m, float* p, LinPad* out, hipStream_t s) {
  for (int l = 0; l < GMPC_MAX_LAYERS; ++l) out->WSP[l] = nullptr;
  if (!sparse_form(dyn.L, dyn.dims, n, m)) return;
  p = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(p) + 1023) & ~(uintptr_t)1023);
  for (int l = 1; l < dyn.L - 1; ++l) {
    out->WSP[l] = p;
    hipLaunchKernelGGL(k_pack_sparse, dim3((GMPC_SP_H * GMPC_SP_H + 255) / 256), dim3(256), 0, s, dyn.W[l], p);
    p += (size_t)(GMPC_SP_H + GMPC_LIN_PADROWS) * GMPC_SP_ROW;
  }
}

// v if bit BIT of w is set, else +0.0f (bit -> all-ones word -> AND, as the seed of k_linearize_regs: written as a
// select, hipcc builds every lane mask first and selects afterwards)
template <int BIT>
__device__ __forceinline__ float keep_if(float v, uint32_t w) {
  unsigned full, vb = __float_as_uint(v);
  asm("v_bfe_i32 %1, %2, %3, 1\n\tv_and_b32 %0, %0, %1" : "+v"(vb), "=&v"(full) : "v"(w), "n"(BIT));
  return __uint_as_float(vb);
}
template <int... J>
__device__ __forceinline__ f32x4 keep_if4(f32x4 v, uint32_t w, std::integer_sequence<int, J...>) {
  return f32x4{keep_if<J>(v[J & 3], w)...};
}
// elements j = 0..3 of v kept where bit B0 + j of w is set
template <int B0>
__device__ __forceinline__ f32x4 keep_if4(f32x4 v, uint32_t w) {
  return keep_if4(v, w, std::integer_sequence<int, B0, B0 + 1, B0 + 2, B0 + 3>{});
}

// LDS: GMPC_SP_WAVE_BYTES per wave, 65.1 KB per workgroup -- two workgroups (eight waves) per CU
// grouped: contiguous sample chunks per wave and rows 16..n-1 in group jobs (needs samp_mul == 1, samp_add == 0);
// otherwise the strided sample split and rows 0..15 only
__global__ __launch_bounds__(GMPC_THREADS, 2) void k_linearize_sparse(
    int NSamp, int T, int n, int m, int Lh, LinPad lp, const uint32_t* masks, const int* active, float* AB,
    int samp_mul, int samp_add, int grouped) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, l16 = lane & 15;
  const int nm = n + m;
  const int nrow = n < 16 ? n : 16;
  char* wbase = smem + wave * GMPC_SP_WAVE_BYTES;
  float* st = reinterpret_cast<float*>(wbase);                                      // S tile [16][STR]
  // unit list (32-bit entries: no 16-bit extensions) and its [CAP][2] even / odd split for the tail tile
  unsigned* lk = reinterpret_cast<unsigned*>(wbase + 16 * GMPC_SP_STR * 4);
  unsigned* lt = lk + GMPC_SP_CAP;
  // zero units 200..207 of the S tile (never written again)
  if (lane < 16 * 8) st[(lane >> 3) * GMPC_SP_STR + GMPC_SP_H + (lane & 7)] = 0.f;
  if (lane + 64 < 16 * 8) st[((lane + 64) >> 3) * GMPC_SP_STR + GMPC_SP_H + (lane & 7)] = 0.f;

  // lane constants (bytes): A operands of units 16 t + l16 in a packed W^T row; the tail tile's unit 192 + (l16 & 7);
  // the S tile column of this lane's Jacobian row; its list half for the tail tile
  const int lw = l16 * 16, lwt = (192 + (l16 & 7)) * 4;
  const int ls = l16 * GMPC_SP_STR * 4;
  const int tsel = l16 >= 8 ? 1 : 0;
  const unsigned* lkl = lk + g;                    // this lane's entry 4 p + g: lkl[4 p], its tail half: ltl_[8 p]
  const unsigned* ltl_ = lt + 2 * g + tsel;
  // seed operand: W_L[k][l16]; the rows past n read past the end of the buffer, which returns zero
  const int lsn = l16 < n ? l16 * 4 : (1 << 28);
  const __amdgpu_buffer_rsrc_t rsl = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(lp.WLP), 0, (GMPC_SP_H + GMPC_LIN_PADROWS) * n * (int)sizeof(float), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs0 = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(lp.WTP[0]), 0, (GMPC_SP_H + GMPC_LIN_PADROWS) * 32 * (int)sizeof(float), 0x00020000);

  // One job.  GRP = false: rows 0..15 of sample s, every column of the tiles is that sample.  GRP = true: row jr of
  // the cnt <= 16 consecutive samples s.., one per column (s + cnt <= NSamp); a column past cnt or of a trajectory
  // that is not active has an all-zero mask and is not stored.
  auto job = [&](auto grpc, int s, int jr, int cnt) __attribute__((always_inline)) {
    constexpr bool GRP = decltype(grpc)::value;
    bool cvalid = true;                    // GRP: this lane's column is a live sample
    size_t sid = (size_t)s * samp_mul + samp_add;
    if constexpr (GRP) {
      cvalid = l16 < cnt;
      if (cvalid) sid = (size_t)s + l16;
      if (cvalid && active != nullptr) cvalid = active[sid / T] != 0;
      if (__ballot(cvalid) == 0ull) return;
    } else {
      if (active != nullptr && active[sid / T] == 0) return;
    }
    const uint32_t* mrow = masks + sid * Lh * GMPC_MW;

    // relu words 0..6 of hidden layer ml for this lane's column (GRP; word 6 cut to units 192..199)
    auto colwords = [&](int ml, uint32_t (&w)[7]) {
#pragma unroll
      for (int i = 0; i < 7; ++i) w[i] = cvalid ? mrow[ml * GMPC_MW + i] : 0u;
      w[6] &= 0xFFu;
    };
    // wave-uniform relu words of the job's list for layer ml: the sample's, or the union over the 16 columns
    auto listwords = [&](int ml, uint32_t (&w)[7]) {
      if constexpr (GRP) {
        colwords(ml, w);
#pragma unroll
        for (int i = 0; i < 7; ++i) {
#pragma unroll
          for (int d = 1; d < 16; d <<= 1) w[i] |= (uint32_t)__shfl_xor((int)w[i], d);
          w[i] = __builtin_amdgcn_readfirstlane(w[i]);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 7; ++i) w[i] = __builtin_amdgcn_readfirstlane(mrow[ml * GMPC_MW + i]);
      }
    };

    // active list of hidden layer ml: returns its length.  Entries from the length on, as far as the k-steps and the
    // loads that run ahead reach (4 np + 12), point at the zero unit
    auto build = [&](int ml) -> int {
      __builtin_amdgcn_wave_barrier();
      uint32_t mw[7];
      listwords(ml, mw);
      int base = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t lo = mw[2 * c];
        uint32_t hi = c < 3 ? mw[2 * c + 1] : 0u;
        const uint32_t lo_m = c < 3 ? lo : (lo & 0xFFu);     // units 192..199 of word 6
        const uint32_t word = lane < 32 ? lo_m : hi;
        const int pos = base + (int)__builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo_m, 0u));
        const unsigned u = 64 * c + lane;
        if ((word >> (lane & 31)) & 1u) {
          const bool odd = (u & 1u) != 0;
          lk[pos] = u;
          *reinterpret_cast<v2u*>(lt + 2 * pos) = v2u{odd ? GMPC_SP_Z : u, odd ? u : GMPC_SP_Z};
        }
        base += __builtin_popcount(lo_m) + __builtin_popcount(hi);
      }
      if (lane < 16) {
        lk[base + lane] = GMPC_SP_Z;
        *reinterpret_cast<v2u*>(lt + 2 * (base + lane)) = v2u{GMPC_SP_Z, GMPC_SP_Z};
      }
      __builtin_amdgcn_wave_barrier();
      return base;
    };

    // ---- hidden GEMMs  S_{l-1} = W_l S_l over the active units of S_l,  l = Lh-1 .. 1 (seed: S = W_L)
    auto layer = [&](int l, auto seedc) __attribute__((always_inline)) {
      constexpr bool seed = decltype(seedc)::value;
      const int np = (build(l) + 3) >> 2;
      const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<float*>(lp.WSP[l]), 0, (GMPC_SP_H + GMPC_LIN_PADROWS) * GMPC_SP_ROW * 4, 0x00020000);
      f32x4 acc[13];
      // GRP: relu words of the layer this GEMM produces, for this lane's column (used in the hand-over), moved so
      // that bit 16 hh + j of word nt is unit 32 nt + 16 hh + 4 g + j
      uint32_t cw[7];
      if constexpr (GRP) {
        colwords(l - 1, cw);
#pragma unroll
        for (int i = 0; i < 6; ++i) cw[i] >>= 4 * g;
        cw[6] >>= 4 * (g & 1);
      }
      struct Ops { float w[13]; float b; unsigned k, kt; };
      Ops r[GMPC_SP_RD];
      auto tables = [&](Ops& o, int p) {
        o.k = lkl[4 * p];
        o.kt = ltl_[8 * p];
      };
      auto loads = [&](Ops& o) {
        const int k = (int)o.k, kt = (int)o.kt;
        const int vo = (k << 10) + lw, vt = (kt << 10) + lwt;
        // tile 4 q + j: units 16 (4 q + j) + l16
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const v4u a = __builtin_amdgcn_raw_buffer_load_b128(wrs, vo + 256 * q, 0, 0);
          o.w[4 * q] = __uint_as_float(a.x); o.w[4 * q + 1] = __uint_as_float(a.y);
          o.w[4 * q + 2] = __uint_as_float(a.z); o.w[4 * q + 3] = __uint_as_float(a.w);
        }
        o.w[12] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wrs, vt, 0, 0));
        if constexpr (seed) o.b = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsl, k * n * 4 + lsn, 0, 0));
        else o.b = st[(ls >> 2) + k];
      };
      auto step = [&](int p, Ops& cur, Ops& ahead2) __attribute__((always_inline)) {
        loads(ahead2);                 // k-step p + 2 (its list entries were read at k-step p - 1)
        tables(cur, p + 3);            // cur's entries were last used for its loads at k-step p - 2
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < 13; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.w[t], cur.b, acc[t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      };
      if (np == 0) {
#pragma unroll
        for (int t = 0; t < 13; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      } else {
        tables(r[0], 0); tables(r[1], 1); tables(r[2], 2);
        loads(r[0]); loads(r[1]);
        // k-step 0 starts the chains from the constant zero (no accumulator initialisation on the vector port)
        loads(r[2]);
        tables(r[0], 3);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < 13; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(r[0].w[t], r[0].b, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        // whole groups of three k-steps with one exit, then the last one or two (the accumulators stay in place)
        int p = 1;
        for (; p + 3 <= np; p += 3) {
          step(p, r[1], r[0]);
          step(p + 1, r[2], r[1]);
          step(p + 2, r[0], r[2]);
        }
        if (p < np) step(p, r[1], r[0]);
        if (p + 1 < np) step(p + 1, r[2], r[1]);
      }
      mfma_fence<false>(acc[0], acc[1], acc[2], acc[3], acc[4], acc[5], acc[6], acc[7], acc[8], acc[9], acc[10],
                        acc[11], acc[12]);
      __builtin_amdgcn_wave_barrier();
      // GRP: the list of the next GEMM is a union, so an output of a unit this column's sample has inactive is read
      // there: it becomes the exact +0 the dense chain's relu select leaves (both tail partials: 0 + 0)
      if constexpr (GRP) {
        acc[0] = keep_if4<0>(acc[0], cw[0]); acc[1] = keep_if4<16>(acc[1], cw[0]);
        acc[2] = keep_if4<0>(acc[2], cw[1]); acc[3] = keep_if4<16>(acc[3], cw[1]);
        acc[4] = keep_if4<0>(acc[4], cw[2]); acc[5] = keep_if4<16>(acc[5], cw[2]);
        acc[6] = keep_if4<0>(acc[6], cw[3]); acc[7] = keep_if4<16>(acc[7], cw[3]);
        acc[8] = keep_if4<0>(acc[8], cw[4]); acc[9] = keep_if4<16>(acc[9], cw[4]);
        acc[10] = keep_if4<0>(acc[10], cw[5]); acc[11] = keep_if4<16>(acc[11], cw[5]);
        acc[12] = keep_if4<0>(acc[12], cw[6]);
      }
      // accumulator rows 4 g + j of tile 2 nt + hh = units 32 nt + 16 hh + 4 g + j, column = this lane's row
      float* srow = st + l16 * GMPC_SP_STR;
#pragma unroll
      for (int t = 0; t < 12; ++t)
        *reinterpret_cast<f32x4*>(srow + 32 * (t >> 1) + 16 * (t & 1) + 4 * g) = acc[t];
      // tail: rows 0..7 even-k partials of units 192..199, rows 8..15 the odd-k ones (to 208..215)
      *reinterpret_cast<f32x4*>(srow + (g < 2 ? 192 : 200) + 4 * g) = acc[12];
      __builtin_amdgcn_wave_barrier();
      if (g < 2) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(srow + 192 + 4 * g);
        const f32x4 y = *reinterpret_cast<const f32x4*>(srow + 208 + 4 * g);
        *reinterpret_cast<f32x4*>(srow + 192 + 4 * g) = x + y;
      }
      __builtin_amdgcn_wave_barrier();
    };
    if constexpr (GRP) {
      // seed through the S tile: S[column][u] = W_L[u][jr] where the column's sample has unit u of layer Lh-1 active,
      // else +0; the first GEMM then reads it over the union list like every other
      __builtin_amdgcn_wave_barrier();
      float* srow = st + l16 * GMPC_SP_STR + 4 * g;
      const uint32_t* mcol = mrow + (Lh - 1) * GMPC_MW;
      const int wo = (4 * g * n + jr) * 4;                 // W_L[4 g][jr], bytes
      // units 32 nt + 16 hh + 4 g + j: bit 16 hh + j of word nt moved down by 4 g (a rolled loop: unrolled, the 50
      // loads and their addresses are all live at once)
#pragma unroll 1
      for (int nt = 0; nt < 6; ++nt) {
        const uint32_t cw = (cvalid ? mcol[nt] : 0u) >> (4 * g);
        f32x4 v0, v1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v0[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsl, wo + (32 * nt + j) * n * 4, 0, 0));
          v1[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsl, wo + (32 * nt + 16 + j) * n * 4, 0, 0));
        }
        *reinterpret_cast<f32x4*>(srow + 32 * nt) = keep_if4<0>(v0, cw);
        *reinterpret_cast<f32x4*>(srow + 32 * nt + 16) = keep_if4<16>(v1, cw);
      }
      if (g < 2) {                                         // units 192..199
        const uint32_t cw = (cvalid ? mcol[6] & 0xFFu : 0u) >> (4 * g);
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          v[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsl, wo + (192 + j) * n * 4, 0, 0));
        *reinterpret_cast<f32x4*>(srow + 192) = keep_if4<0>(v, cw);
      }
      __builtin_amdgcn_wave_barrier();
      for (int l = Lh - 1; l >= 1; --l) layer(l, std::false_type{});
    } else {
      layer(Lh - 1, std::true_type{});
      for (int l = Lh - 2; l >= 1; --l) layer(l, std::false_type{});
    }

    // ---- input GEMM  out = W_1 S_1 over the active units of S_1: coordinates 16 t + l16 of W_1^T's 32-wide rows
    {
      const int np = (build(0) + 3) >> 2;
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      const bool two = nm > 16;      // (both tiles always run: W_1^T rows are 32 wide, zero padded)
      struct Ops0 { float w0, w1, b; unsigned k; };
      Ops0 r[GMPC_SP_RD];
      auto tables = [&](Ops0& o, int p) { o.k = lkl[4 * p]; };
      auto loads = [&](Ops0& o) {
        const int vo = (int)(o.k << 7) + l16 * 4;
        o.w0 = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs0, vo, 0, 0));
        o.w1 = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs0, vo + 64, 0, 0));
        o.b = st[(ls >> 2) + o.k];
      };
      auto step = [&](int p, Ops0& cur, Ops0& ahead2) __attribute__((always_inline)) {
        loads(ahead2);
        tables(cur, p + 3);
        __builtin_amdgcn_sched_barrier(0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.w0, cur.b, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.w1, cur.b, acc1, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      };
      tables(r[0], 0); tables(r[1], 1); tables(r[2], 2);
      loads(r[0]); loads(r[1]);
      int p = 0;
      for (; p + 3 <= np; p += 3) {
        step(p, r[0], r[2]);
        step(p + 1, r[1], r[0]);
        step(p + 2, r[2], r[1]);
      }
      if (p < np) step(p, r[0], r[2]);
      if (p + 1 < np) step(p + 1, r[1], r[0]);
      mfma_fence<false>(acc0, acc1);
      // this lane's column: Jacobian row l16 of sample s, or row jr of sample s + l16
      const int orow = GRP ? jr : l16;
      if (GRP ? cvalid : l16 < nrow) {
        float* dst = AB + ((size_t)(GRP ? s + l16 : s) * n + orow) * nm;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c = 4 * g + j;
          if (c < nm) dst[c] = acc0[j] + (c == orow ? 1.0f : 0.0f);
          if (two && c + 16 < nm) dst[c + 16] = acc1[j] + (c + 16 == orow ? 1.0f : 0.0f);
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
  };

  constexpr int WPB = GMPC_THREADS / 64;
  const int w = blockIdx.x * WPB + wave, W = gridDim.x * WPB;
  if (!grouped) {
    for (int s = w; s < NSamp; s += W) job(std::false_type{}, s, 0, 0);
    return;
  }
  // wave w: samples [c0, c1), a contiguous chunk of C (the last ones shorter or empty), so that consecutive time
  // steps of a trajectory -- whose relu masks differ in a few units only -- share the tiles of a group job
  const int C = (NSamp + W - 1) / W;
  const long c0l = (long)w * C;
  const int c0 = c0l < NSamp ? (int)c0l : NSamp;
  const int len = NSamp - c0 < C ? NSamp - c0 : C;
  for (int s = c0; s < c0 + len; ++s) job(std::false_type{}, s, 0, 0);
  // rows 16..n-1: the chunk cut into near-equal groups of at most 16 consecutive samples
  if (n > 16 && len > 0) {
    const int ng = (len + 15) >> 4;
    for (int r = 16; r < n; ++r)
      for (int i = 0; i < ng; ++i) {
        const int a = i * len / ng, b = (i + 1) * len / ng;
        job(std::true_type{}, c0 + a, r, b - a);
      }
  }
}

// what the launcher below tests before it launches anything (host only)
bool gmpc_linearize_sparse_covers(long NSamp, int n, int m, int L, const int* dims, bool strided) {
  if (!sparse_form(L, dims, n, m)) return false;
  // a strided sample set sends rows 16..n-1 to the dense chain's row window
  return !(n > 16 && strided) || gmpc_linearize_regs_covers(NSamp, n, m, L, dims, 16);
}

int gmpc_launch_linearize_sparse(int NSamp, int T, int n, int m, const MlpDesc& dyn, const LinPad& lp,
                                 const uint32_t* masks, const int* active, float* AB, int samp_mul, int samp_add,
                                 hipStream_t s) {
  const int Lh = dyn.L - 1;
  if (!sparse_form(dyn.L, dyn.dims, n, m) || lp.NT != 7 || lp.NTF != 1 || lp.NGF != 1) return -1;
  if (NSamp <= 0) return 0;
  // rows 16..n-1 run inside the kernel as group jobs over consecutive samples; a strided sample set has none, its
  // rows 16..n-1 go to the dense chain's row window first (any error leaves nothing launched)
  const int grouped = samp_mul == 1 && samp_add == 0;
  if (n > 16 && !grouped &&
      gmpc_launch_linearize_regs_rows(NSamp, T, n, m, dyn, lp, masks, active, AB, samp_mul, samp_add, 16, s) != 0)
    return -1;
  const size_t lds = (size_t)(GMPC_THREADS / 64) * GMPC_SP_WAVE_BYTES;
  int grid = (NSamp + 3) / 4;
  if (grid > 256 * 2) grid = 256 * 2;      // persistent: two workgroups per CU
  hipLaunchKernelGGL(k_linearize_sparse, dim3(grid), dim3(GMPC_THREADS), lds, s, NSamp, T, n, m, Lh, lp, masks,
                     active, AB, samp_mul, samp_add, grouped);
  return 0;
}
