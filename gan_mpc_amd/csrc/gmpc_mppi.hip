// Model-predictive path integral control on the sampled rollouts of the cross-entropy method (gmpc_mppi_solve,
// gmpc_mppi_vjp).  The samples and their costs are CEM's (k_sampled_rollout over CemDrawn, the sampler of
// gmpc_cem_sampler.h); the elite cut becomes the softmax weights w_s = exp(-(J_s - J_min) / lambda), so the update is
// a smooth function of the costs and has a derivative.
//
//   k_mppi_update     one workgroup per problem: J_min over the finite costs, the weights in LDS, then one (step,
//                     control) per thread: sum_s w_s and sum_s w_s u_s in sample order, the controls regenerated
//                     (for T m < 256 by the whole workgroup, in blocks of samples staged in LDS: the same sums).
//   k_mppi_cotangent  (backward) one workgroup per problem of a chunk: the samples of the iteration regenerated as
//                     rows of the chunk workspace, a_s = <g, u_s - new_mean>, the cost cotangents c_s over each row's
//                     T + 1 costs, x0 and the goals replicated per row: the operands of the rollout and its VJP.
//   k_mppi_reduce     (backward) one workgroup per problem of a chunk: the masked sums over the samples of the VJP's
//                     rows, in sample order, into g, grad_x0 and grad_goal.
// No atomics; every sum has an order that depends on neither B nor the launch geometry.
#include "gmpc_cem_sampler.h"

#include <cstring>

#define GMPC_MPPI_MAX_N 4096      // samples per problem (the weights: 16 KiB of LDS)
#define GMPC_MPPI_STAGE_FLOATS 8192   // k_mppi_update's staged products (32 KiB of LDS)

// min over the workgroup, the same value in every thread (a min does not depend on its order); red: 4 floats
__device__ __forceinline__ float mppi_block_min(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  __syncthreads();      // (red may still be read from an earlier call)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
}

// w[s] = exp(-(J_s - J_min) / lam) of one problem's costs, 0 for a NaN or an infinite cost; returns J_min (+inf: no
// finite cost, every weight 0).  The caller synchronises before reading w.
__device__ __forceinline__ float mppi_weights(const float* costs, int N, float lam, float* w, float* red) {
  float mn = INFINITY;
  for (int i = threadIdx.x; i < N; i += GMPC_THREADS) {
    const float c = costs[i];
    if (fabsf(c) < INFINITY) mn = fminf(mn, c);
  }
  mn = mppi_block_min(mn, red);
  for (int i = threadIdx.x; i < N; i += GMPC_THREADS) {
    const float c = costs[i];
    w[i] = fabsf(c) < INFINITY ? expf(-((c - mn) / lam)) : 0.f;
  }
  return mn;
}

// sum of the weights in sample order (every thread computes the same value: broadcast reads of LDS)
__device__ __forceinline__ float mppi_weight_sum(const float* w, int N) {
  float sw = 0.f;
  for (int s = 0; s < N; ++s) sw = __fadd_rn(sw, w[s]);
  return sw;
}

__global__ __launch_bounds__(GMPC_THREADS) void k_mppi_update(MppiUpdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_mu[];
  float* w = reinterpret_cast<float*>(smem_mu);     // [N]
  __shared__ float red[4];
  const int tid = threadIdx.x, b = blockIdx.x, N = a.N, T = a.T, m = a.m;
  const float* costs = a.costs + (size_t)b * N;
  const float mn = mppi_weights(costs, N, a.lam, w, red);
  __syncthreads();
  if (a.costs_copy)
    for (int i = tid; i < N; i += GMPC_THREADS) a.costs_copy[(size_t)b * N + i] = costs[i];
  const bool alive = mn < INFINITY;
  const float sw = alive ? mppi_weight_sum(w, N) : 1.f;     // (>= 1: the cheapest sample's weight is 1)
  if (a.weights)
    for (int i = tid; i < N; i += GMPC_THREADS) a.weights[(size_t)b * N + i] = w[i] / sw;
  const float g = a.gamma, g1 = 1.f - a.gamma;
  const int Tm = T * m;
  if (a.stage > 0) {
    // Fewer elements than threads (T m < 256): one element per thread would leave most of the workgroup idle behind
    // N Philox calls each.  Blocks of a.stage samples instead: every thread forms products w_s u_s into LDS, then
    // thread e adds its column in sample order -- the same products in the same order as the loop below.
    float* prod = w + N;     // [a.stage][Tm]
    const size_t o = (size_t)b * Tm + tid;
    float mu = 0.f, su = 0.f;
    if (tid < Tm) {
      mu = a.mean[o];
      if (a.mean_trace) a.mean_trace[o] = mu;
    }
    if (!alive) return;      // no finite cost: the mean stays, bit for bit
    for (int s0 = 0; s0 < N; s0 += a.stage) {
      const int cnt = min(a.stage, N - s0);
      for (int i = tid; i < cnt * Tm; i += GMPC_THREADS) {
        const int k = i / Tm, e = i - k * Tm, t = e / m, j = e - t * m;
        const float ws = w[s0 + k];
        const float lo = a.lo ? a.lo[j] : -INFINITY, hi = a.hi ? a.hi[j] : INFINITY;
        const size_t oe = (size_t)b * Tm + e;
        prod[i] = ws == 0.f ? 0.f
                            : __fmul_rn(ws, cem_control(a.rng, b, s0 + k, t, j, m, a.mean[oe], a.sd[oe], lo, hi));
      }
      __syncthreads();
      if (tid < Tm)
        for (int k = 0; k < cnt; ++k)
          if (w[s0 + k] != 0.f) su = __fadd_rn(su, prod[k * Tm + tid]);
      __syncthreads();
    }
    // (behind the last barrier: every read of a.mean has been made)
    if (tid < Tm) a.mean[o] = __fadd_rn(__fmul_rn(g, mu), __fmul_rn(g1, su / sw));
    return;
  }
  for (int e = tid; e < Tm; e += GMPC_THREADS) {
    const int t = e / m, j = e - t * m;
    const size_t o = (size_t)b * Tm + e;
    const float mu = a.mean[o];
    if (a.mean_trace) a.mean_trace[o] = mu;
    if (!alive) continue;     // no finite cost: the mean stays, bit for bit
    const float sg = a.sd[o];
    const float lo = a.lo ? a.lo[j] : -INFINITY, hi = a.hi ? a.hi[j] : INFINITY;
    float su = 0.f;
    for (int s = 0; s < N; ++s) {
      const float ws = w[s];
      if (ws != 0.f) su = __fadd_rn(su, __fmul_rn(ws, cem_control(a.rng, b, s, t, j, m, mu, sg, lo, hi)));
    }
    a.mean[o] = __fadd_rn(__fmul_rn(g, mu), __fmul_rn(g1, su / sw));
  }
}

// ---- the backward pass ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(GMPC_THREADS) void k_mppi_cotangent(MppiCotArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_mc[];
  float* w = reinterpret_cast<float*>(smem_mc);     // [N]
  __shared__ float red[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int bc = blockIdx.x, b = a.b0 + bc, N = a.N, T = a.T, m = a.m, n = a.n, Tm = T * m;
  const size_t r0 = (size_t)bc * N;     // the problem's first row of the chunk
  const float mn = mppi_weights(a.costs + (size_t)b * N, N, a.lam, w, red);
  __syncthreads();
  const bool alive = mn < INFINITY;
  const float sw = alive ? mppi_weight_sum(w, N) : 1.f;
  // the samples, as the forward pass formed them
  const float* mean = a.mean + (size_t)b * Tm;
  const float* sd = a.sd + (size_t)b * Tm;
  for (int i = tid; i < N * Tm; i += GMPC_THREADS) {
    const int s = i / Tm, e = i - s * Tm, t = e / m, j = e - t * m;
    const float lo = a.lo ? a.lo[j] : -INFINITY, hi = a.hi ? a.hi[j] : INFINITY;
    a.Us[r0 * Tm + i] = cem_control(a.rng, b, s, t, j, m, mean[e], sd[e], lo, hi);
  }
  __syncthreads();      // (a workgroup's own global writes are visible to it behind the barrier)
  // new_mean = sum_s w~_s u_s, in sample order
  float* nm = a.nm + (size_t)bc * Tm;
  for (int e = tid; e < Tm; e += GMPC_THREADS) {
    float su = 0.f;
    for (int s = 0; s < N; ++s) {
      const float ws = w[s];
      if (ws != 0.f) su = __fadd_rn(su, __fmul_rn(ws, a.Us[(r0 + s) * Tm + e]));
    }
    nm[e] = su / sw;
  }
  __syncthreads();
  // a_s = <g, u_s - new_mean> (one wave per sample, lanes over the elements), c_s over the row's T + 1 costs
  const float* g = a.g + (size_t)b * Tm;
  const float cf = -(1.f - a.gamma) / a.lam;
  for (int s = wave; s < N; s += GMPC_THREADS / 64) {
    float as = 0.f;
    for (int e = lane; e < Tm; e += 64) as = fmaf(g[e], a.Us[(r0 + s) * Tm + e] - nm[e], as);
    as = wave_sum(as);
    const float wn = alive ? w[s] / sw : 0.f;
    const float cs = wn != 0.f ? cf * wn * as : 0.f;
    for (int t = lane; t <= T; t += 64) a.gc[(r0 + s) * (T + 1) + t] = cs;
    if (lane == 0) a.wn[r0 + s] = wn;
  }
  // x0 and the goals of the problem, once per row
  const float* x0 = a.x0 + (size_t)b * n;
  for (int i = tid; i < N * n; i += GMPC_THREADS) a.x0r[r0 * n + i] = x0[i % n];
  const int gn = (T + 1) * n;
  const float* goal = a.goal + (size_t)b * gn;
  for (int e = tid; e < gn; e += GMPC_THREADS) {
    const float v = goal[e];
    for (int s = 0; s < N; ++s) a.goalr[(r0 + s) * gn + e] = v;
  }
}

__global__ __launch_bounds__(GMPC_THREADS) void k_mppi_reduce(MppiRedArgs a) {
  const int tid = threadIdx.x, bc = blockIdx.x, b = a.b0 + bc, N = a.N, T = a.T, m = a.m, n = a.n, Tm = T * m;
  const size_t r0 = (size_t)bc * N;
  const float* wn = a.wn + r0;
  const float gam = a.gamma, g1 = 1.f - a.gamma;
  // g <- gamma g + sum_s mask_s ((1 - gamma) w~_s g + GU_s): a clamped control does not move with the mean
  for (int e = tid; e < Tm; e += GMPC_THREADS) {
    const int j = e % m;
    const float lo = a.lo ? a.lo[j] : -INFINITY, hi = a.hi ? a.hi[j] : INFINITY;
    const float ge = a.g[(size_t)b * Tm + e];
    float acc = 0.f;
    for (int s = 0; s < N; ++s) {
      const float ws = wn[s];
      if (ws == 0.f) continue;
      const float u = a.Us[(r0 + s) * Tm + e];
      if (u > lo && u < hi) acc = __fadd_rn(acc, fmaf(g1 * ws, ge, a.GU[(r0 + s) * Tm + e]));
    }
    a.g[(size_t)b * Tm + e] = fmaf(gam, ge, acc);
  }
  if (a.gx0)
    for (int i = tid; i < n; i += GMPC_THREADS) {
      float acc = a.gx0[(size_t)b * n + i];
      for (int s = 0; s < N; ++s)
        if (wn[s] != 0.f) acc = __fadd_rn(acc, a.Gx0[(r0 + s) * n + i]);
      a.gx0[(size_t)b * n + i] = acc;
    }
  if (a.ggoal) {
    const int gn = (T + 1) * n;
    for (int e = tid; e < gn; e += GMPC_THREADS) {
      float acc = a.ggoal[(size_t)b * gn + e];
      for (int s = 0; s < N; ++s)
        if (wn[s] != 0.f) acc = __fadd_rn(acc, a.Ggoal[(r0 + s) * gn + e]);
      a.ggoal[(size_t)b * gn + e] = acc;
    }
  }
}

// out[i] += v[i / cols], or (set) out[i] = v[i / cols]: the sums across chunks and iterations, and a row broadcast
__global__ __launch_bounds__(GMPC_THREADS) void k_mppi_add(long count, int cols, const float* v, float* out, int set) {
  const long i = (long)blockIdx.x * GMPC_THREADS + threadIdx.x;
  if (i >= count) return;
  const float x = v[i / cols];
  out[i] = set ? x : out[i] + x;
}

// Host-side launchers ---------------------------------------------------------------------------
int gmpc_launch_mppi_update(const MppiUpdArgs& a0, hipStream_t s) {
  if (a0.N < 1 || a0.N > GMPC_MPPI_MAX_N || !(a0.lam > 0.f)) return 1;
  MppiUpdArgs a = a0;
  const int Tm = a.T * a.m;
  // samples per staged block: up to 32 KiB of products (0: T m >= 256, one element per thread keeps every thread busy)
  a.stage = Tm < GMPC_THREADS ? min(a.N, GMPC_MPPI_STAGE_FLOATS / Tm) : 0;
  const size_t lds = ((size_t)a.N + (size_t)a.stage * Tm) * sizeof(float);
  hipLaunchKernelGGL(k_mppi_update, dim3(a.B), dim3(GMPC_THREADS), lds, s, a);
  return 0;
}

int gmpc_launch_mppi_cotangent(const MppiCotArgs& a, hipStream_t s) {
  if (a.N < 1 || a.N > GMPC_MPPI_MAX_N || !(a.lam > 0.f) || a.Bc < 1) return 1;
  hipLaunchKernelGGL(k_mppi_cotangent, dim3(a.Bc), dim3(GMPC_THREADS), (size_t)a.N * sizeof(float), s, a);
  return 0;
}

void gmpc_launch_mppi_reduce(const MppiRedArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_mppi_reduce, dim3(a.Bc), dim3(GMPC_THREADS), 0, s, a);
}

void gmpc_launch_mppi_add(long count, const float* v, float* out, hipStream_t s) {
  if (count < 1) return;
  hipLaunchKernelGGL(k_mppi_add, dim3((unsigned)((count + GMPC_THREADS - 1) / GMPC_THREADS)), dim3(GMPC_THREADS), 0, s,
                     count, 1, v, out, 0);
}

void gmpc_launch_mppi_bcast(int rows, int cols, const float* v, float* out, hipStream_t s) {
  const long count = (long)rows * cols;
  hipLaunchKernelGGL(k_mppi_add, dim3((unsigned)((count + GMPC_THREADS - 1) / GMPC_THREADS)), dim3(GMPC_THREADS), 0, s,
                     count, cols, v, out, 1);
}
