// The packed bf16 weight images of the sampled rollouts in bf16 mode (gmpc_set_sampled_precision; DESIGN.md section
// 23): the BF16 instantiations of k_sampled_rollout (gmpc_cem_rollout.h) read them through dg_gemm_bf16
// (gmpc_dg_gemm.h, where the layout is stated).
//
//   k_pack_bf16   one thread per 16-byte group (8 k-consecutive values of one column) of one layer's image: the fp32
//                 weights rounded to bf16, to nearest even, a NaN kept; zeros in the padding of K and N.  One launch for
//                 every layer of both MLPs (blockIdx.y: the layer).
#include "gmpc_dg_gemm.h"

struct PackArgs {
  int nl;                                   // layers of both MLPs
  int K[2 * GMPC_MAX_LAYERS], N[2 * GMPC_MAX_LAYERS];
  const float* W[2 * GMPC_MAX_LAYERS];      // [K][N] row-major
  __bf16* img[2 * GMPC_MAX_LAYERS];         // [Kp / 8][Np][8]
};

__global__ __launch_bounds__(GMPC_THREADS) void k_pack_bf16(PackArgs a) {
  const int l = blockIdx.y, K = a.K[l], N = a.N[l], Np = dg_np(N), groups = (dg_kp(K) >> 3) * Np;
  const float* __restrict__ W = a.W[l];
  bf16x8_t* img = reinterpret_cast<bf16x8_t*>(a.img[l]);
  for (int g = blockIdx.x * GMPC_THREADS + threadIdx.x; g < groups; g += gridDim.x * GMPC_THREADS) {
    const int kb = g / Np, j = g - kb * Np;
    bf16x8_t v;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = 8 * kb + i;
      v[i] = static_cast<__bf16>(k < K && j < N ? W[(size_t)k * N + j] : 0.f);
    }
    img[g] = v;
  }
}

// Host side --------------------------------------------------------------------------------------------------------
size_t gmpc_bf16_image_elems(int L, const int* dims) {
  size_t e = 0;
  for (int l = 0; l < L; ++l) e += (size_t)dg_kp(dims[l]) * dg_np(dims[l + 1]);
  return e;
}

// img: src's dims and biases, W[l] the layers' images laid one behind the other from `base` (16-byte aligned: every
// image is a multiple of 8 elements)
void gmpc_bind_bf16_images(MlpDesc& img, const MlpDesc& src, void* base) {
  img = src;
  __bf16* p = static_cast<__bf16*>(base);
  for (int l = 0; l < src.L; ++l) {
    img.W[l] = reinterpret_cast<const float*>(p);
    img.WT[l] = nullptr;
    p += (size_t)dg_kp(src.dims[l]) * dg_np(src.dims[l + 1]);
  }
}

void gmpc_launch_pack_bf16(const MlpDesc& dyn, const MlpDesc& dyn_img, const MlpDesc& cost, const MlpDesc& cost_img,
                           hipStream_t s) {
  PackArgs a;
  a.nl = 0;
  int most = 1;
  const MlpDesc* src[2] = {&dyn, &cost};
  const MlpDesc* dst[2] = {&dyn_img, &cost_img};
  for (int w = 0; w < 2; ++w)
    for (int l = 0; l < src[w]->L; ++l) {
      const int i = a.nl++;
      a.K[i] = src[w]->dims[l];
      a.N[i] = src[w]->dims[l + 1];
      a.W[i] = src[w]->W[l];
      a.img[i] = reinterpret_cast<__bf16*>(const_cast<float*>(dst[w]->W[l]));
      const int groups = (dg_kp(a.K[i]) >> 3) * dg_np(a.N[i]);
      most = groups > most ? groups : most;
    }
  hipLaunchKernelGGL(k_pack_bf16, dim3((most + GMPC_THREADS - 1) / GMPC_THREADS, a.nl), dim3(GMPC_THREADS), 0, s, a);
}
