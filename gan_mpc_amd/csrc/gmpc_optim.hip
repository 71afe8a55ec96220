// Optimiser and utility kernels: fixed-order sums, global-norm clip + Adam (gan/runner.py:51-63), the Polyak blend
// and the matrix transposes (one matrix, or a list of them in one launch).
#include "gmpc_launch.h"

// Single-block sum of `count` floats (fixed order: thread-strided partials, then tree in LDS).
__global__ __launch_bounds__(1024) void k_sum(int count, const float* v, float* out, int square) {
  __shared__ float sh[1024];
  float s = 0.f;
  for (int e = threadIdx.x; e < count; e += blockDim.x) {
    const float x = v[e];
    s += square ? x * x : x;
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sh[0];
}

// two-stage sum of squares of (grad * scale): partials per block, then k_sum
__global__ __launch_bounds__(GMPC_THREADS) void k_sqsum_part(long count, const float* g, float scale,
                                                             float* part) {
  __shared__ float sh[GMPC_THREADS];
  float s = 0.f;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < count;
       e += (long)gridDim.x * blockDim.x) {
    const float x = g[e] * scale;
    s = fmaf(x, x, s);
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = GMPC_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

// optax clip_by_global_norm + adam (gan/runner.py:58): g <- g*scale; if !(norm < max_norm)
// g <- g / norm * max_norm; m,v update; p += -lr * mhat / (sqrt(vhat) + eps)
// `sqpart`: the 256 partial sums of k_sqsum_part; every block adds them up itself -- the tree of k_sum over the same
// values, so the norm has the bits it had when a k_sum launch stood between the two kernels (one launch and one
// dependent kernel boundary less on the tail of every step)
__global__ __launch_bounds__(256) void k_adam(long count, float* p, const float* g, float* m, float* v, float scale,
                                              const float* sqpart, float max_norm, float lr, float b1, float b2,
                                              float omb1, float omb2, float eps, float bc1, float bc2) {
  __shared__ float sh[256];
  sh[threadIdx.x] = sqpart[threadIdx.x];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  const float gn = sqrtf(sh[0]);
  float x = g[e] * scale;
  if (!(gn < max_norm)) x = x / gn * max_norm;
  const float mn = b1 * m[e] + omb1 * x;
  const float vn = b2 * v[e] + omb2 * x * x;
  m[e] = mn;
  v[e] = vn;
  const float mh = mn / bc1, vh = vn / bc2;
  p[e] = p[e] + (-lr * mh / (sqrtf(vh) + eps));
}

// Polyak blend (norm/cost_trainer.py:88-92): out = f * prev + (1 - f) * cur
__global__ void k_polyak(long count, const float* prev, const float* cur, float f, float omf,
                         float* out) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < count) out[e] = f * prev[e] + omf * cur[e];
}

__global__ void k_transpose(int R, int C, const float* in, float* out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= R * C) return;
  const int r = e / C, c = e - r * C;
  out[(size_t)c * R + r] = in[e];
}

// every transpose of a list in one launch: blockIdx.z = matrix, 32 x 32 tiles through LDS (both the read and the write
// are coalesced)
__global__ __launch_bounds__(256) void k_transpose_all(TransposeList d) {
  __shared__ float tile[32][33];
  const int mt = blockIdx.z;
  const int R = d.R[mt], C = d.C[mt];
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  if (r0 >= R || c0 >= C) return;
  const float* in = d.in[mt];
  float* out = d.out[mt];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8)
    if (r0 + r < R && c0 + tx < C) tile[r][tx] = in[(size_t)(r0 + r) * C + c0 + tx];
  __syncthreads();
  for (int cc = ty; cc < 32; cc += 8)
    if (c0 + cc < C && r0 + tx < R) out[(size_t)(c0 + cc) * R + r0 + tx] = tile[tx][cc];
}

// ---------------------------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------------------------
void gmpc_launch_sum(int count, const float* v, float* out, int square, hipStream_t s) {
  hipLaunchKernelGGL(k_sum, dim3(1), dim3(1024), 0, s, count, v, out, square);
}

void gmpc_launch_adam(long count, float* p, const float* g, float* m, float* v, float scale,
                      int step, double lr, double max_norm, double b1, double b2, double eps,
                      float* scratch /* >= 257 floats */, hipStream_t s) {
  const int nb = 256;
  hipLaunchKernelGGL(k_sqsum_part, dim3(nb), dim3(GMPC_THREADS), 0, s, count, g, scale, scratch + 1);
  const float bc1 = (float)(1.0 - pow(b1, (double)step)), bc2 = (float)(1.0 - pow(b2, (double)step));
  hipLaunchKernelGGL(k_adam, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, count, p, g, m, v,
                     scale, scratch + 1, (float)max_norm, (float)lr, (float)b1, (float)b2,
                     (float)(1.0 - b1), (float)(1.0 - b2), (float)eps, bc1, bc2);
}

void gmpc_launch_polyak(long count, const float* prev, const float* cur, double f, float* out,
                        hipStream_t s) {
  hipLaunchKernelGGL(k_polyak, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, count, prev, cur,
                     (float)f, (float)(1.0 - f), out);
}

void gmpc_launch_transpose(int R, int C, const float* in, float* out, hipStream_t s) {
  if ((long)R * C > (1L << 16)) {     // large activations: the tiled form
    TransposeList one{};
    one.nm = 1; one.R[0] = R; one.C[0] = C; one.in[0] = in; one.out[0] = out;
    gmpc_launch_transpose_all(one, s);
    return;
  }
  const int cnt = R * C;
  hipLaunchKernelGGL(k_transpose, dim3((cnt + 255) / 256), dim3(256), 0, s, R, C, in, out);
}

void gmpc_launch_transpose_all(const TransposeList& mats, hipStream_t s) {
  int rmax = 1, cmax = 1;
  for (int i = 0; i < mats.nm; ++i) {
    rmax = mats.R[i] > rmax ? mats.R[i] : rmax;
    cmax = mats.C[i] > cmax ? mats.C[i] : cmax;
  }
  hipLaunchKernelGGL(k_transpose_all, dim3((cmax + 31) / 32, (rmax + 31) / 32, mats.nm), dim3(256), 0, s, mats);
}

void gmpc_launch_mlp_transpose_all(const MlpDesc& d, hipStream_t s) {
  TransposeList mats{};
  mats.nm = d.L;
  for (int l = 0; l < d.L; ++l) {
    mats.R[l] = d.dims[l]; mats.C[l] = d.dims[l + 1];
    mats.in[l] = d.W[l]; mats.out[l] = const_cast<float*>(d.WT[l]);
  }
  gmpc_launch_transpose_all(mats, s);
}
