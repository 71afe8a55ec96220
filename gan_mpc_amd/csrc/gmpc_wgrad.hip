// Weight-gradient GEMMs: C[M][N] = sum_r A[r][:M]^T B[r][:N] over the rows of a batch, with the bias column sums
// beside them (the contract is in gmpc_launch.h).  Used by the critic step, the dynamics regression, the expert
// trainer and the bilevel / rollout gradients.  Three forms: the LDS-tiled VALU kernel (any shape), the matrix-core
// kernel (N % 32 == 0), and the batch kernel that covers the problems of one optimiser step in one launch.  All of them
// write partial sums per row chunk and add them in chunk order, so every result is run-to-run identical.
#include "gmpc_launch.h"

// C[M][N] (+ colsum) partials: Cp[split][M][N] = sum over a row chunk of A[r][:M]^T B[r][:N].
// 64x64 tile per workgroup, 4x4 micro-tile per thread, 16 rows per LDS stage.
__global__ __launch_bounds__(GMPC_THREADS) void k_wgrad(int rows, int M, int N, const float* A,
                                                        int lda, const float* Bm, int ldb,
                                                        int rows_per_split, float* Cp,
                                                        float* colsum_p, int cs_rows) {
  __shared__ float As[16][64 + 4];
  __shared__ float Bs[16][64 + 4];
  const int tid = threadIdx.x;
  const int tm = blockIdx.x * 64, tn = blockIdx.y * 64, sp = blockIdx.z;
  const int r0 = sp * rows_per_split, r1 = min(rows, r0 + rows_per_split);
  const int ty = tid / 16, tx = tid % 16;   // micro-tile rows ty*4.., cols tx*4..
  float acc[4][4] = {};
  float csum[4] = {0.f, 0.f, 0.f, 0.f};
  const bool do_cs = (colsum_p != nullptr) && (blockIdx.x == 0);
  for (int rb = r0; rb < r1; rb += 16) {
    for (int e = tid; e < 16 * 64; e += blockDim.x) {
      const int rr = e / 64, cidx = e % 64;
      const int r = rb + rr;
      As[rr][cidx] = (r < r1 && tm + cidx < M) ? A[(size_t)r * lda + tm + cidx] : 0.f;
      Bs[rr][cidx] = (r < r1 && tn + cidx < N) ? Bm[(size_t)r * ldb + tn + cidx] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
      float av[4], bv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { av[i] = As[rr][ty * 4 + i]; bv[i] = Bs[rr][tx * 4 + i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
      if (do_cs && ty == 0 && rb + rr < cs_rows) {
#pragma unroll
        for (int j = 0; j < 4; ++j) csum[j] += bv[j];
      }
    }
    __syncthreads();
  }
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      const int mm = tm + ty * 4 + i, nn = tn + tx * 4 + j;
      if (mm < M && nn < N) Cp[((size_t)sp * M + mm) * N + nn] = acc[i][j];
    }
  if (do_cs && ty == 0)
    for (int j = 0; j < 4; ++j) {
      const int nn = tn + tx * 4 + j;
      if (nn < N) colsum_p[(size_t)sp * N + nn] = csum[j];
    }
}

// out[e] = sum_sp part[sp][e], deterministic: 64 elements per block, the splits are shared by 4
// thread groups, each keeping 8 independent partial sums (so 8 loads are in flight per thread);
// the fixed combination order makes the result run-to-run identical.
__global__ __launch_bounds__(256) void k_reduce_splits(int count, int nsplit, const float* part,
                                                       float* out) {
  __shared__ float sh[4][64];
  const int el = threadIdx.x & 63, seg = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + el;
  const int q = (nsplit + 3) / 4;
  const int s0 = seg * q, s1 = min(nsplit, s0 + q);
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (e < count) {
    int sp = s0;
    for (; sp + 8 <= s1; sp += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] += part[(size_t)(sp + u) * count + e];
    }
    for (; sp < s1; ++sp) a[0] += part[(size_t)sp * count + e];
  }
  sh[seg][el] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  __syncthreads();
  if (seg == 0 && e < count) out[e] = (sh[0][el] + sh[1][el]) + (sh[2][el] + sh[3][el]);
}

// ---------------------------------------------------------------------------------------------
// Weight-gradient GEMM on the matrix cores: C[M][N] = sum_r A[r][:M]^T B[r][:N] with both operands
// read straight from global memory in their natural row-major layout (the MFMA A operand of k-step
// r is row r of A, the B operand row r of B: both coalesced).  One wavefront owns a 32 x 32*NTW
// strip of C over one chunk of rows; partial strips are summed in chunk order (deterministic).
// Requires N % (32*NTW) == 0 and B followed by GMPC_WGRAD_PAD allocated, finite rows (gmpc_launch.h: they meet a
// zero A operand); A is clamped (it may be a caller's buffer).  On the transposed route (gmpc_wgrad_route_of) the
// launcher passes the caller's B as this A and the caller's A as this B: the pad rows are then wanted behind the
// caller's A.  v_mfma_f32_32x32x2_f32 = k-ordered exact fp32 fmaf chain.
// ---------------------------------------------------------------------------------------------
template <int NTW>
__global__ __launch_bounds__(GMPC_THREADS) void k_wgrad_mfma(int rows, int M, int N, const float* A,
                                                             int lda, const float* Bm, int ldb,
                                                             int rows_per_chunk, float* Cp) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const int mstrips = (M + 31) >> 5, ngroups = N / (32 * NTW);
  const int nchunks = (rows + rows_per_chunk - 1) / rows_per_chunk;
  const int total = mstrips * ngroups * nchunks;
  const int item = blockIdx.x * (GMPC_THREADS / 64) + wave;
  if (item >= total) return;
  const int chunk = item / (mstrips * ngroups);
  const int rem = item - chunk * mstrips * ngroups;
  const int mi = rem / ngroups, ng = rem - mi * ngroups;
  const int r0 = chunk * rows_per_chunk;
  const int r1 = min(rows, r0 + rows_per_chunk);
  const int Kp = (r1 - r0 + 1) & ~1;
  const int acol = mi * 32 + l31;
  const bool aok = acol < M;
  const float* ap = A + (aok ? acol : M - 1);
  auto afn = [&](int k0) -> float {
    const int r = r0 + k0 + half;
    const float v = ap[(size_t)min(r, rows - 1) * lda];
    return (aok && r < r1) ? v : 0.f;
  };
  f32x16 acc[NTW];
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) acc[nt][rg] = 0.f;
  const float* bp0 = Bm + (size_t)(r0 + half) * ldb + ng * 32 * NTW + l31;
  gemm_tile<NTW>(bp0, ldb, Kp, afn, acc);
  float* cp = Cp + (size_t)chunk * M * N;
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt) {
    const int col = ng * 32 * NTW + nt * 32 + l31;
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) {
      const int row = mi * 32 + (rg & 3) + 8 * (rg >> 2) + 4 * half;
      if (row < M) cp[(size_t)row * N + col] = acc[nt][rg];
    }
  }
}

// column sums of the first cs_rows rows of B: partial[chunk][j]
__global__ __launch_bounds__(GMPC_THREADS) void k_colsum(int cs_rows, int N, const float* Bm, int ldb,
                                                         int rows_per_chunk, float* part) {
  const int chunk = blockIdx.x;
  const int r0 = chunk * rows_per_chunk, r1 = min(cs_rows, r0 + rows_per_chunk);
  for (int j = threadIdx.x; j < N; j += blockDim.x) {
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int r = r0;
    for (; r + 8 <= r1; r += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] += Bm[(size_t)(r + u) * ldb + j];
    }
    for (; r < r1; ++r) a[0] += Bm[(size_t)r * ldb + j];
    part[(size_t)chunk * N + j] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  }
}

// ---------------------------------------------------------------------------------------------
// Batched weight gradients: the five or six row-sum GEMMs of one optimiser step (LSTM input and
// recurrent kernels, head layers) differ only in their operands, and each is far too small to fill
// the chip (a few hundred wave-tiles): issued one by one they cost a launch, a tail and a reduction
// launch each.  Here ONE launch covers the wave-tiles of all problems plus their bias column sums
// (the trailing workgroups), and ONE launch reduces all the partial sums, in the same fixed chunk
// order as before (deterministic).  Problems need N % 128 == 0 (32 * GMPC_WG_NTW columns per wave), rows >= 64, ldb % 4 == 0
// and a 16-byte aligned B; a problem with M == 0 is its column sums alone (any N and ldb).
// ---------------------------------------------------------------------------------------------
// C(32 x 256) += A^T B over Kp rows for one wave: row r of A / B is the MFMA A / B operand of k-step r / 2.
// B goes through 16-byte loads: lane l31 holds columns 4 l31 .. 4 l31 + 3 of each 128-column half, so tile j
// of the accumulator is columns 128 (j >> 2) + 4 l31 + (j & 3) (the store undoes the permutation); the
// operands of D k-steps are in flight.  Measured (LSTM + head problems of the headline step, batch kernel +
// reductions): 8 tiles / ring 3 / dword loads 0.227 ms; 8 tiles, ring 8 or 12, one wave per SIMD 0.232;
// 8 tiles, ring 4, two waves 0.183; 4 tiles, ring 4, four waves 0.172 -- the rows stream from HBM and it
// is occupancy, not ring depth, that hides their latency.
template <int D, int NTW, typename AF>
__device__ __forceinline__ void wgrad_tile_x4(const float* __restrict__ bp0, int ldb, int Kp, AF afn,
                                              f32x16 (&acc)[NTW]) {
  static_assert(NTW == 4 || NTW == 8, "one or two 16-byte loads per lane and k-step");
  float4 b[D][NTW / 4];
  float a[D];
  const int nks = Kp >> 1;
  auto load = [&](int slot, int ks) {
    const float4* bp = reinterpret_cast<const float4*>(bp0 + (size_t)2 * ks * ldb);
    b[slot][0] = bp[0];
    if (NTW > 4) b[slot][NTW / 4 - 1] = bp[32];
    a[slot] = afn(2 * ks);
  };
#pragma unroll
  for (int j = 0; j < D - 1; ++j)
    if (j < nks) load(j, j);
  for (int k0 = 0; k0 < nks; k0 += D) {
#pragma unroll
    for (int u = 0; u < D; ++u) {
      const int ks = k0 + u;
      if (ks + D - 1 < nks) load((u + D - 1) % D, ks + D - 1);
      __builtin_amdgcn_sched_barrier(0);
      if (ks < nks) {
        const float av = a[u];
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[u][0].x, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[u][0].y, acc[1], 0, 0, 0);
        acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[u][0].z, acc[2], 0, 0, 0);
        acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[u][0].w, acc[3], 0, 0, 0);
        if (NTW > 4) {
          acc[NTW - 4] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[u][NTW / 4 - 1].x, acc[NTW - 4], 0, 0, 0);
          acc[NTW - 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[u][NTW / 4 - 1].y, acc[NTW - 3], 0, 0, 0);
          acc[NTW - 2] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[u][NTW / 4 - 1].z, acc[NTW - 2], 0, 0, 0);
          acc[NTW - 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[u][NTW / 4 - 1].w, acc[NTW - 1], 0, 0, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

#ifndef GMPC_WG_RING
#define GMPC_WG_RING 4     // k-steps of operands in flight per wave
#endif
#ifndef GMPC_WG_OCC
#define GMPC_WG_OCC 4      // waves per SIMD: the rows stream from HBM, occupancy hides what the ring does not
#endif
#ifndef GMPC_WG_NTW
#define GMPC_WG_NTW 4      // 32-column tiles per wave item (64 accumulator registers)
#endif
__global__ __launch_bounds__(GMPC_THREADS, GMPC_WG_OCC) void k_wgrad_batch(WgBatch bt, float* part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if ((int)blockIdx.x >= bt.gemm_blocks) {
    // bias column sums: one workgroup per (problem, row chunk)
    const int cb = blockIdx.x - bt.gemm_blocks;
    int pi = -1;
    for (int i = 0; i < bt.np; ++i)
      if (cb >= bt.p[i].cs_block0 && cb < bt.p[i].cs_block0 + bt.p[i].cchunks) pi = i;
    if (pi < 0) return;
    const WgProb& q = bt.p[pi];
    const int chunk = cb - q.cs_block0;
    const int r0 = chunk * q.crpc, r1 = min(q.cs_rows, r0 + q.crpc);
    float* out = part + q.cs_part_off + (size_t)chunk * q.N;
    for (int j = threadIdx.x; j < q.N; j += blockDim.x) {
      float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      int r = r0;
      for (; r + 8 <= r1; r += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] += q.B[(size_t)(r + u) * q.ldb + j];
      }
      for (; r < r1; ++r) a[0] += q.B[(size_t)r * q.ldb + j];
      out[j] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    }
    return;
  }
  constexpr int NTW = GMPC_WG_NTW;
  const int item = blockIdx.x * (GMPC_THREADS / 64) + wave;
  int pi = 0;
  for (int i = 1; i < bt.np; ++i)
    if (item >= bt.p[i].item0) pi = i;
  const WgProb& q = bt.p[pi];
  const int local = item - q.item0;
  if (local >= q.mstrips * q.ngroups * q.nchunks) return;
  const int half = lane >> 5, l31 = lane & 31;
  const int chunk = local / (q.mstrips * q.ngroups);
  const int rem = local - chunk * q.mstrips * q.ngroups;
  const int mi = rem / q.ngroups, ng = rem - mi * q.ngroups;
  const int rows = q.rows, M = q.M, N = q.N;
  const int r0 = chunk * q.rpc;
  const int r1 = min(rows, r0 + q.rpc);
  const int Kp = (r1 - r0 + 1) & ~1;
  const int acol = mi * 32 + l31;
  const bool aok = acol < M;
  const float* ap = q.A + (aok ? acol : M - 1);
  const int lda = q.lda;
  auto afn = [&](int k0) -> float {
    const int r = r0 + k0 + half;
    const float v = ap[(size_t)min(r, rows - 1) * lda];
    return (aok && r < r1) ? v : 0.f;
  };
  f32x16 acc[NTW];
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) acc[nt][rg] = 0.f;
  // (rows past the chunk meet a zero A operand; the B reads stay inside the array: the last chunk's
  // odd tail row is clamped by the row pointer below)
  const float* bp0 = q.B + (size_t)(r0 + half) * q.ldb + ng * 32 * NTW + 4 * l31;
  if (r0 + Kp > rows) {      // wave-uniform
    // the chunk's last k-step would read row `rows`: run it from a clamped pointer
    wgrad_tile_x4<GMPC_WG_RING, NTW>(bp0, q.ldb, Kp - 2, afn, acc);
    const float* bl = q.B + (size_t)min(r0 + Kp - 2 + half, rows - 1) * q.ldb + ng * 32 * NTW + 4 * l31;
    auto afl = [&](int k0) -> float { return afn(k0 + Kp - 2); };
    wgrad_tile_x4<1, NTW>(bl, q.ldb, 2, afl, acc);
  } else {
    wgrad_tile_x4<GMPC_WG_RING, NTW>(bp0, q.ldb, Kp, afn, acc);
  }
  // tiles 4 j .. 4 j + 3 of a lane are four consecutive columns: one 16-byte store per accumulator row (N % 128 == 0
  // and the partial buffer's slices are multiples of 4 floats, so the address is aligned)
  float* cp = part + q.part_off + (size_t)chunk * M * N;
#pragma unroll
  for (int j = 0; j < NTW / 4; ++j) {
    const int col = ng * 32 * NTW + j * 128 + 4 * l31;
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) {
      const int row = mi * 32 + (rg & 3) + 8 * (rg >> 2) + 4 * half;
      if (row < M)
        *reinterpret_cast<float4*>(cp + (size_t)row * N + col) =
            make_float4(acc[4 * j][rg], acc[4 * j + 1][rg], acc[4 * j + 2][rg], acc[4 * j + 3][rg]);
    }
  }
}

// all reductions of a batch: blocks [red_block0, ...) of problem i sum its nchunks partial C's,
// blocks [cs_red_block0, ...) its column-sum partials; same arithmetic as k_reduce_splits
__global__ __launch_bounds__(256) void k_reduce_batch(WgBatch bt, const float* part) {
  __shared__ float sh[4][64];
  int pi = 0, kind = 0;
  for (int i = 0; i < bt.np; ++i) {
    const int b_ = (int)blockIdx.x;
    if (b_ >= bt.p[i].red_block0 && b_ < bt.p[i].cs_red_block0) { pi = i; kind = 0; }
    if (bt.p[i].colsum != nullptr && b_ >= bt.p[i].cs_red_block0 &&
        b_ < bt.p[i].cs_red_block0 + (bt.p[i].N + 63) / 64) { pi = i; kind = 1; }
  }
  const WgProb& q = bt.p[pi];
  const int count = kind == 0 ? q.M * q.N : q.N;
  const int nsplit = kind == 0 ? q.nchunks : q.cchunks;
  const float* src = part + (kind == 0 ? q.part_off : q.cs_part_off);
  float* out = kind == 0 ? q.C : q.colsum;
  const int blk = blockIdx.x - (kind == 0 ? q.red_block0 : q.cs_red_block0);
  const int el = threadIdx.x & 63, seg = threadIdx.x >> 6;
  const int e = blk * 64 + el;
  const int qn = (nsplit + 3) / 4;
  const int s0 = seg * qn, s1 = min(nsplit, s0 + qn);
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (e < count) {
    int sp = s0;
    for (; sp + 8 <= s1; sp += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] += src[(size_t)(sp + u) * count + e];
    }
    for (; sp < s1; ++sp) a[0] += src[(size_t)sp * count + e];
  }
  sh[seg][el] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  __syncthreads();
  if (seg == 0 && e < count) out[e] = (sh[0][el] + sh[1][el]) + (sh[2][el] + sh[3][el]);
}

// ---------------------------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------------------------
// Row chunks of a column sum over cs_rows rows: about 64 rows each, at most `cap` chunks and at most as many as fit
// part_floats (<= 0: unbounded) with N floats each; one empty chunk when there are no rows (the sum is zero).
static void colsum_chunks(int cs_rows, int N, long part_floats, int cap, int& crpc, int& cchunks) {
  cchunks = (cs_rows + 63) / 64;
  if (cchunks > cap) cchunks = cap;
  if (part_floats > 0 && (long)cchunks * N > part_floats) cchunks = (int)(part_floats / N);
  if (cchunks < 1) cchunks = 1;
  crpc = (cs_rows + cchunks - 1) / cchunks;
  if (crpc < 1) crpc = 1;
  cchunks = (cs_rows + crpc - 1) / crpc;
  if (cchunks < 1) cchunks = 1;
}

static void launch_colsum_chunks(int cs_rows, int N, const float* Bm, int ldb, float* colsum, float* part, int crpc,
                                 int cchunks, hipStream_t s) {
  hipLaunchKernelGGL(k_colsum, dim3(cchunks), dim3(GMPC_THREADS), 0, s, cs_rows, N, Bm, ldb, crpc, part);
  hipLaunchKernelGGL(k_reduce_splits, dim3((N + 63) / 64), dim3(256), 0, s, N, cchunks, part, colsum);
}

bool gmpc_launch_colsum(int rows, int N, const float* Bm, int ldb, float* colsum, float* part, long part_floats,
                        hipStream_t s) {
  if (part_floats > 0 && part_floats < N) return false;
  const WgradRoute r = gmpc_wgrad_route_of(rows, 0, N, true, rows, part_floats, false);
  launch_colsum_chunks(rows, N, Bm, ldb, colsum, part, r.crpc, r.cchunks, s);
  return true;
}

int gmpc_wgrad_batch_plan(WgProb* probs, int np, long part_floats) {
  if (np < 1 || np > GMPC_WG_MAX) return 0;
  for (int i = 0; i < np; ++i) {
    WgProb& q = probs[i];
    if (q.M == 0 && q.colsum != nullptr) {      // column sums only (no GEMM part)
      q.mstrips = 0;
      q.ngroups = 0;
      continue;
    }
    if (q.N % (32 * GMPC_WG_NTW) != 0 || q.rows < 64 || q.ldb % 4 != 0 || (reinterpret_cast<uintptr_t>(q.B) & 15) != 0)
      return 0;
    q.mstrips = (q.M + 31) / 32;
    q.ngroups = q.N / (32 * GMPC_WG_NTW);
  }
  // one chunk length (rows per wave-tile) for all problems, so that every wave does the same amount
  // of work: the shortest one whose partial sums fit the buffer and that needs <= 4096 wave-tiles
  static const int rpcs[] = {64, 96, 128, 192, 256, 384, 512, 768, 1024, 2048, 4096, 8192, 1 << 30};
  constexpr long max_items = 4096;
  int rpc = 0;
  for (int cand : rpcs) {
    long need = 0, items = 0;
    for (int i = 0; i < np; ++i) {
      const WgProb& q = probs[i];
      const long nch = (q.rows + cand - 1) / cand;
      need += nch * q.M * q.N + (q.colsum ? 1024L * q.N : 0);
      items += nch * q.mstrips * q.ngroups;
    }
    if (need <= part_floats && items <= max_items) { rpc = cand; break; }
  }
  if (rpc == 0) return 0;
  int item = 0, cs_blocks = 0, red_blocks = 0;
  long off = 0;
  for (int i = 0; i < np; ++i) {
    WgProb& q = probs[i];
    q.rpc = rpc;
    q.nchunks = (q.rows + rpc - 1) / rpc;
    q.item0 = item;
    item += q.mstrips * q.ngroups * q.nchunks;
    q.part_off = off;
    off += (long)q.nchunks * q.M * q.N;
    if (q.colsum != nullptr) {
      colsum_chunks(q.cs_rows, q.N, 0, 1024, q.crpc, q.cchunks);
      q.cs_block0 = cs_blocks;
      cs_blocks += q.cchunks;
      q.cs_part_off = off;
      off += (long)q.cchunks * q.N;
    } else {
      q.cchunks = 0; q.crpc = 0; q.cs_block0 = cs_blocks; q.cs_part_off = off;
    }
    off = (off + 3) & ~3L;               // every slice starts on a 16-byte boundary (float4 stores of the partials)
    q.red_block0 = red_blocks;
    red_blocks += (q.M * q.N + 63) / 64;
    q.cs_red_block0 = red_blocks;
    if (q.colsum != nullptr) red_blocks += (q.N + 63) / 64;
  }
  return off > part_floats ? 0 : rpc;
}

bool gmpc_launch_wgrad_batch(WgProb* probs, int np, float* part, long part_floats, hipStream_t s) {
  if (gmpc_wgrad_batch_plan(probs, np, part_floats) == 0) return false;
  WgBatch bt;
  bt.np = np;
  int item = 0, cs_blocks = 0, red_blocks = 0;
  for (int i = 0; i < np; ++i) {
    const WgProb& q = probs[i];
    bt.p[i] = q;
    item += q.mstrips * q.ngroups * q.nchunks;
    cs_blocks += q.cchunks;
    red_blocks += (q.M * q.N + 63) / 64 + (q.colsum != nullptr ? (q.N + 63) / 64 : 0);
  }
  bt.gemm_blocks = (item + 3) / 4;
  hipLaunchKernelGGL(k_wgrad_batch, dim3(bt.gemm_blocks + cs_blocks), dim3(GMPC_THREADS), 0, s, bt, part);
  hipLaunchKernelGGL(k_reduce_batch, dim3(red_blocks), dim3(256), 0, s, bt, part);
  return true;
}

// Tiling of the matrix-core form: 32*ntw columns per wave, chunks of >= 64 rows, about 1024 wave-tiles, the chunks
// doubled until their partial sums fit; false when the shape does not qualify or one chunk's partial sum does not fit.
static bool mfma_tiling(int rows, int M, int N, long part_floats, int& ntw, int& rpc, int& nchunks) {
  if (N % 32 != 0 || rows < 64) return false;
  const int nt_all = N / 32;
  ntw = (nt_all % 8 == 0) ? 8 : (nt_all % 4 == 0) ? 4 : (nt_all % 2 == 0) ? 2 : 1;
  const int mstrips = (M + 31) / 32, ngroups = nt_all / ntw;
  nchunks = 1024 / (mstrips * ngroups);
  if (nchunks < 1) nchunks = 1;
  rpc = (rows + nchunks - 1) / nchunks;
  if (rpc < 64) rpc = 64;
  rpc = (rpc + 1) & ~1;
  nchunks = (rows + rpc - 1) / rpc;
  while ((long)nchunks * M * N > part_floats && rpc < rows) {
    rpc *= 2;
    nchunks = (rows + rpc - 1) / rpc;
  }
  return (long)nchunks * M * N <= part_floats;
}

// The decision of gmpc_launch_wgrad (M >= 1) and gmpc_launch_colsum (M == 0) without their launches.
WgradRoute gmpc_wgrad_route_of(int rows, int M, int N, bool colsum, int cs_rows, long part_floats, bool mfma_ok) {
  WgradRoute r{};
  if (M == 0) {
    r.form = WGRAD_COLSUM;
    colsum_chunks(cs_rows, N, part_floats, 2048, r.crpc, r.cchunks);
    return r;
  }
  if (mfma_ok && mfma_tiling(rows, M, N, part_floats, r.ntw, r.rpc, r.nchunks)) {
    r.form = WGRAD_MFMA;
    // the column sums reuse the buffer after the reduction of C (stream order): N <= M * N <= part_floats
    if (colsum) colsum_chunks(cs_rows, N, part_floats, 2048, r.crpc, r.cchunks);
    return r;
  }
  // narrow N (e.g. the critic head's last layer, N = 1): compute C^T = sum_r B_r^T A_r instead;
  // C^T (N x M) has the same memory image as C when N == 1
  if (mfma_ok && N == 1 && M % 32 == 0 && mfma_tiling(rows, 1, M, part_floats, r.ntw, r.rpc, r.nchunks)) {
    r.form = WGRAD_MFMA_SWAPPED;
    if (colsum) colsum_chunks(cs_rows, N, part_floats, 2048, r.crpc, r.cchunks);
    return r;
  }
  r = WgradRoute{};
  r.form = WGRAD_VALU;
  int nsplit = (rows + 511) / 512;
  if (nsplit > GMPC_WGRAD_MAX_SPLIT) nsplit = GMPC_WGRAD_MAX_SPLIT;
  // the partial sums must fit the scratch buffer (wide layers: n + m = 1088 inputs at C5)
  const long per_split = (long)M * N + (colsum ? N : 0);
  if (part_floats > 0 && (long)nsplit * per_split > part_floats) nsplit = (int)(part_floats / per_split);
  if (nsplit < 1) {        // not even one partial sum fits: one split needs no partial sums
    nsplit = 1;
    r.direct = true;
  }
  int rps = (rows + nsplit - 1) / nsplit;
  rps = (rps + 15) / 16 * 16;
  r.rpc = rps;
  r.nchunks = (rows + rps - 1) / rps;
  return r;
}

static void launch_wgrad_mfma(const WgradRoute& r, int rows, int M, int N, const float* A, int lda, const float* Bm,
                              int ldb, float* C, float* part, hipStream_t s) {
  const int total = ((M + 31) / 32) * (N / (32 * r.ntw)) * r.nchunks;
  const dim3 grid((total + 3) / 4), blk(GMPC_THREADS);
  const int rpc = r.rpc;
  switch (r.ntw) {
    case 8: hipLaunchKernelGGL(k_wgrad_mfma<8>, grid, blk, 0, s, rows, M, N, A, lda, Bm, ldb, rpc, part); break;
    case 4: hipLaunchKernelGGL(k_wgrad_mfma<4>, grid, blk, 0, s, rows, M, N, A, lda, Bm, ldb, rpc, part); break;
    case 2: hipLaunchKernelGGL(k_wgrad_mfma<2>, grid, blk, 0, s, rows, M, N, A, lda, Bm, ldb, rpc, part); break;
    default: hipLaunchKernelGGL(k_wgrad_mfma<1>, grid, blk, 0, s, rows, M, N, A, lda, Bm, ldb, rpc, part); break;
  }
  hipLaunchKernelGGL(k_reduce_splits, dim3((M * N + 63) / 64), dim3(256), 0, s, M * N, r.nchunks, part, C);
}

void gmpc_launch_wgrad(int rows, int M, int N, const float* A, int lda, const float* Bm, int ldb,
                       float* C, float* colsum, int cs_rows, float* part, hipStream_t s,
                       long part_floats, bool mfma_ok) {
  const WgradRoute r = gmpc_wgrad_route_of(rows, M, N, colsum != nullptr, cs_rows, part_floats, mfma_ok);
  if (r.form == WGRAD_MFMA || r.form == WGRAD_MFMA_SWAPPED) {
    if (r.form == WGRAD_MFMA) launch_wgrad_mfma(r, rows, M, N, A, lda, Bm, ldb, C, part, s);
    else launch_wgrad_mfma(r, rows, 1, M, Bm, ldb, A, lda, C, part, s);
    if (colsum) launch_colsum_chunks(cs_rows, N, Bm, ldb, colsum, part, r.crpc, r.cchunks, s);
    return;
  }
  const int nsplit = r.nchunks;
  if (r.direct) {
    hipLaunchKernelGGL(k_wgrad, dim3((M + 63) / 64, (N + 63) / 64, 1), dim3(GMPC_THREADS), 0, s, rows, M, N, A, lda, Bm,
                       ldb, r.rpc, C, colsum, cs_rows);
    return;
  }
  float* cpart = part;
  float* cspart = colsum ? part + (size_t)nsplit * M * N : nullptr;
  hipLaunchKernelGGL(k_wgrad, dim3((M + 63) / 64, (N + 63) / 64, nsplit), dim3(GMPC_THREADS), 0, s,
                     rows, M, N, A, lda, Bm, ldb, r.rpc, cpart, cspart, cs_rows);
  hipLaunchKernelGGL(k_reduce_splits, dim3((M * N + 63) / 64), dim3(256), 0, s, M * N, nsplit, cpart,
                     C);
  if (colsum)
    hipLaunchKernelGGL(k_reduce_splits, dim3((N + 63) / 64), dim3(256), 0, s, N, nsplit, cspart,
                       colsum);
}

float* gmpc_launch_wgrad_mlp(int rows, int cs_rows, int L, const int* dims, const float* acts, const float* dels,
                             const MlpRows& r, float* g, float* part, long part_floats, hipStream_t s) {
  for (int l = 0; l < L; ++l) {
    const int M = dims[l], N = dims[l + 1];
    gmpc_launch_wgrad(rows, M, N, acts + r.aoff[l], r.stride, dels + r.doff[l], r.stride, g, g + (long)M * N, cs_rows,
                      part, s, part_floats, true);
    g += (long)M * N + N;
  }
  return g;
}
