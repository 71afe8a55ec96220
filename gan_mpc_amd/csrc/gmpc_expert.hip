// Expert sequence model inference: the behaviour-cloning model that turns the state
// history into the goal states and the initial controls of every MPC solve, i.e. the step right
// before the hot path inside the same batched function (policy/base.py:41-61, policy/eval.py:87-107).
//
// Reference arithmetic: expert/nn.py:43-61 (LSTMCell: x -> OptimizedLSTMCell(F) -> y; next_x =
// MLPCell(y) + x; u = tanh(MLPCell(y))), :23-40 (StackedMLPCell: y = relu(Dense(x))), :10-20
// (MLPCell), expert/expert_model.py:60-91 (teacher-forced pass over the history, then `horizon`
// autoregressive steps).  flax gate order i, f, g, o; zero initial carry.
//
// One 512-thread workgroup owns 4 sequences (float4 components) for all hist + T steps: thread j =
// gate pre-activation j (4F <= 512), the cell update runs as (unit, sequence), then the two heads run
// side by side, the state head on threads 0..255, the action head on 256..511, each thread taking the
// neurons j, j + 256, ... of its head's layer (widths and n up to 1024: the C4 / C5 state sizes).
#include "gmpc_launch.h"

#define GMPC_EX_THREADS 512

__global__ __launch_bounds__(GMPC_EX_THREADS) void k_expert_seq(ExpertArgs a) {
  constexpr int SB = 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const ExpertNet& net = a.net;
  float4* act = reinterpret_cast<float4*>(smem);        // [n + F]: x | h   (LSTM input image)
  float4* gbuf = act + (net.n + net.F);                   // [512] gates
  const int hw = net.hw;                                 // activations per head (>= every head width)
  float4* hA = gbuf + GMPC_EX_THREADS;                  // [2 hw] head activations (x half | u half)
  float4* hB = hA + 2 * hw;                             // [2 hw]
  const int tid = threadIdx.x;
  const int n = net.n, m = net.m, F = net.F, G4 = 4 * F;
  const int s0 = blockIdx.x * SB;
  float* actf = reinterpret_cast<float*>(act);
  float* gbf = reinterpret_cast<float*>(gbuf);
  const int half = tid >> 8, hj = tid & 255;            // head: 0 = state, 1 = action; neuron index
  const MlpDesc& hd = half == 0 ? net.hx : net.hu;
  float c = 0.f;                                        // cell state of (unit tid % F, sequence tid / F)
  for (int e = tid; e < F * SB; e += blockDim.x) actf[n * SB + e] = 0.f;     // h = 0
  const int steps = a.hist + a.T;
  for (int st = 0; st < steps; ++st) {
    // ---- input: history row while teacher-forced; then the model's own prediction (kept in act)
    if (st <= a.hist) {
      // st < hist: history[st]; st == hist: the current state x = history[hist] (eval.py:93-99)
      for (int e = tid; e < n * SB; e += blockDim.x) {
        const int sb = e / n, i = e - sb * n;
        const int s = min(s0 + sb, a.B - 1);
        const float v = a.history[((size_t)s * (a.hist + 1) + st) * n + i];
        actf[i * SB + sb] = v;
        if (st == a.hist && s0 + sb < a.B) a.goal[(size_t)s * (a.T + 1) * n + i] = v;
      }
    }
    __syncthreads();
    // ---- y: LSTM cell or first dense layer
    if (F > 0) {
      if (tid < G4) {
        const float bj = net.bcat[tid];
        float4 acc[1] = {make_float4(bj, bj, bj, bj)};
        dense_rows<1>(net.Wcat, n + F, G4, tid, act, acc);
        float4 v = acc[0];
        if (tid >= 2 * F && tid < 3 * F) { v.x = tanhf(v.x); v.y = tanhf(v.y); v.z = tanhf(v.z); v.w = tanhf(v.w); }
        else { v.x = sigmoidf_(v.x); v.y = sigmoidf_(v.y); v.z = sigmoidf_(v.z); v.w = sigmoidf_(v.w); }
        gbuf[tid] = v;
      }
      __syncthreads();
      if (tid < F * SB) {
        const int u = tid % F, sb = tid / F;
        const float ig = gbf[(0 * F + u) * SB + sb], fg = gbf[(1 * F + u) * SB + sb];
        const float gg = gbf[(2 * F + u) * SB + sb], og = gbf[(3 * F + u) * SB + sb];
        c = fg * c + ig * gg;
        const float h = og * tanhf(c);
        actf[(n + u) * SB + sb] = h;
      }
      __syncthreads();
      // both heads read y = h
      if (hj < F) hA[half * hw + hj] = act[n + hj];
    } else {
      const int H0 = net.Y;
      if (tid < H0) {
        const float bj = net.bcat[tid];
        float4 acc[1] = {make_float4(bj, bj, bj, bj)};
        dense_rows<1>(net.Wcat, n, H0, tid, act, acc);
        const float4 v = make_float4(fmaxf(acc[0].x, 0.f), fmaxf(acc[0].y, 0.f), fmaxf(acc[0].z, 0.f),
                                     fmaxf(acc[0].w, 0.f));
        hA[tid] = v;
        hA[hw + tid] = v;
      }
    }
    __syncthreads();
    // ---- heads (same depth): state head on threads 0..255, action head on 256..511
    float4* in = hA;
    float4* out = hB;
    const int L = net.hx.L;
    for (int l = 0; l < L; ++l) {
      const int K = hd.dims[l], N = hd.dims[l + 1];
      for (int j = hj; j < N; j += 256) {
        const float bj = hd.b[l][j];
        float4 acc[1] = {make_float4(bj, bj, bj, bj)};
        dense_rows<1>(hd.W[l], K, N, j, in + half * hw, acc);
        float4 v = acc[0];
        if (l < L - 1) {
          v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
        }
        out[half * hw + j] = v;
      }
      __syncthreads();
      float4* tmp = in; in = out; out = tmp;
    }
    // ---- outputs: next_x = head_x + x (the next input), u = tanh(head_u)
    const bool emit = st >= a.hist;
    const int t = st - a.hist;
    if (half == 0) {
      for (int j = hj; j < n; j += 256) {
        const float4 x = act[j], o = in[j];
        const float4 v = make_float4(o.x + x.x, o.y + x.y, o.z + x.z, o.w + x.w);
        act[j] = v;          // own element: read above, written here, by the same thread
        if (emit) {
#pragma unroll
          for (int cc = 0; cc < 4; ++cc)
            if (s0 + cc < a.B) a.goal[((size_t)(s0 + cc) * (a.T + 1) + t + 1) * n + j] = f4get(v, cc);
        }
      }
    } else if (emit) {
      for (int j = hj; j < m; j += 256) {
        const float4 o = in[hw + j];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
          if (s0 + cc < a.B) a.U[((size_t)(s0 + cc) * a.T + t) * m + j] = tanhf(f4get(o, cc));
      }
    }
    __syncthreads();
  }
}

int gmpc_launch_expert(const ExpertArgs& a0, hipStream_t s) {
  ExpertArgs a = a0;
  ExpertNet& e = a.net;
  if (e.n > 1024 || e.m > 1024 || 4 * e.F > GMPC_EX_THREADS) return -1;
  if (e.hx.L != e.hu.L || e.hx.L < 1) return -1;
  if (e.F == 0 && e.Y > GMPC_EX_THREADS) return -1;      // MLP variant: one first-layer unit per thread
  if (e.hw > 1024) return -1;
  if (e.hw < 256) e.hw = 256;
  const size_t lds = ((size_t)(e.n + e.F) + GMPC_EX_THREADS + 4 * (size_t)e.hw) * sizeof(float4);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_expert_seq),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipGetLastError();
    attr = true;
  }
  if (lds > 159 * 1024) return -1;
  hipLaunchKernelGGL(k_expert_seq, dim3((a.B + 3) / 4), dim3(GMPC_EX_THREADS), lds, s, a);
  return 0;
}
