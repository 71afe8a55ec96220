// Expert sequence model training: loss and gradient of a minibatch of expert windows.
//
// Reference arithmetic: expert/trainer.py:10-31 (calculate_loss under jax.value_and_grad), the model of
// expert/nn.py:10-61 (LSTMCell: x_in -> OptimizedLSTMCell(F) -> y, next_x = MLPCell(y) + x_in,
// u = tanh(MLPCell(y)); StackedMLPCell: y = relu(Dense(x_in))), utils.py:231-240 (discounted_sum: the
// discount is built by repeated fp32 multiplication).  Per sequence, from the zero carry:
//   x_in_t = teacher_forcing ? xseq[t] : next_x_{t-1}   (x_in_0 = xseq[0])
//   loss   = sum_t g^t (|u_t - useq[t]|^2 + |next_x_t - next_xseq[t]|^2)
// The LSTM carry is fed back under teacher forcing too, so BPTT runs through it in both modes; the input
// path (residual + heads) reaches earlier steps only when teacher forcing is off.
//
// k_expert_fit: one 256-thread workgroup per sequence runs the S-step forward and then BPTT in reverse
// time.  It emits, per row r = b*S + t, the row operands of the weight-gradient GEMMs into the context's call
// workspace, at the columns of ExpertNet (bind_expert, gmpc_ctx.h):
//   acts row: [x_in (n) | h_prev (F, LSTM only) | y (Y) | head_x inputs a_1..a_{L-1} | head_u inputs ...]
//   dels row: [dz (4F) or d y_pre (Y) | head_x output deltas d_1..d_L | head_u output deltas d_1..d_L]
//   save row: [activated gates (4F) | c_prev (F) | tanh(c') (F)  (LSTM only) | next_x (n) | u (m)]
// The weight gradients are then sum_r acts^T dels on the matrix cores (gmpc_launch_wgrad: k_wgrad_mfma,
// fixed chunk order), written straight into the flat expert layout.  No atomics anywhere: identical calls
// give identical bits.
#include "gmpc_launch.h"

__device__ __forceinline__ float efit_block_sum(float v, float* red) {
  v = wave_sum(v);
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(GMPC_THREADS) void k_expert_fit(ExpertFitArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem_ef[];
  const ExpertNet& net = a.net;
  const int n = net.n, m = net.m, F = net.F, Y = net.Y, G4 = 4 * F, S = a.S, hw = net.hw, L = net.hx.L;
  const int G = F > 0 ? G4 : Y;           // width of the first layer's output delta
  float* xin = reinterpret_cast<float*>(smem_ef);   // n
  float* lam = xin + n;                             // n   d loss / d next_x through the next input
  float* hs = lam + n;                              // F   carry h
  float* cs = hs + F;                               // F   carry c
  float* dhv = cs + F;                              // F
  float* dcv = dhv + F;                             // F
  float* zg = dcv + F;                              // G   gates (forward), first-layer delta (backward)
  float* yv = zg + G;                               // Y   y (forward), d loss / d y (backward)
  float* hA = yv + Y;                               // 2 hw  x half | u half
  float* hB = hA + 2 * hw;                          // 2 hw
  __shared__ float red[4];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int so = F > 0 ? 6 * F : 0;                 // save offset of next_x
  const int ay = n + F;                             // acts offset of y
  for (int j = tid; j < F; j += GMPC_THREADS) { hs[j] = 0.f; cs[j] = 0.f; }
  float lsum = 0.f, disc = 1.f;
  for (int t = 0; t < S; ++t) {
    const size_t row = (size_t)b * S + t;
    float* arow = a.acts + row * net.stride;
    float* sv = a.save + row * a.sstride;
    if (t == 0 || a.teacher_forcing)
      for (int i = tid; i < n; i += GMPC_THREADS) xin[i] = a.xseq[row * n + i];
    __syncthreads();
    if (a.grad) {
      for (int i = tid; i < n; i += GMPC_THREADS) arow[i] = xin[i];
      for (int j = tid; j < F; j += GMPC_THREADS) { arow[n + j] = hs[j]; sv[G4 + j] = cs[j]; }
    }
    // ---- y: LSTM cell (gates i, f, g, o) or the first dense layer + relu
    if (F > 0) {
      for (int j = tid; j < G4; j += GMPC_THREADS) {
        float acc = net.bcat[j];
        for (int k = 0; k < n; ++k) acc = fmaf(xin[k], net.Wcat[(size_t)k * G4 + j], acc);
        for (int k = 0; k < F; ++k) acc = fmaf(hs[k], net.Wcat[(size_t)(n + k) * G4 + j], acc);
        zg[j] = (j >= 2 * F && j < 3 * F) ? tanhf(acc) : sigmoidf_(acc);
      }
      __syncthreads();
      for (int j = tid; j < F; j += GMPC_THREADS) {
        const float ig = zg[j], fg = zg[F + j], gg = zg[2 * F + j], og = zg[3 * F + j];
        const float c = fg * cs[j] + ig * gg;
        const float tc = tanhf(c);
        const float h = og * tc;
        cs[j] = c;
        hs[j] = h;
        yv[j] = h;
        if (a.grad) {
          sv[j] = ig; sv[F + j] = fg; sv[2 * F + j] = gg; sv[3 * F + j] = og; sv[5 * F + j] = tc;
          arow[ay + j] = h;
        }
      }
    } else {
      for (int j = tid; j < Y; j += GMPC_THREADS) {
        float acc = net.bcat[j];
        for (int k = 0; k < n; ++k) acc = fmaf(xin[k], net.Wcat[(size_t)k * Y + j], acc);
        const float y = fmaxf(acc, 0.f);
        yv[j] = y;
        if (a.grad) arow[ay + j] = y;
      }
    }
    __syncthreads();
    // ---- both heads side by side: neuron e < Nx of the state head, e - Nx of the action head
    const float* inx = yv;
    const float* inu = yv;
    float* out = hA;
    float* other = hB;
    for (int l = 0; l < L; ++l) {
      const int Kx = net.hx.dims[l], Nx = net.hx.dims[l + 1], Ku = net.hu.dims[l], Nu = net.hu.dims[l + 1];
      for (int e = tid; e < Nx + Nu; e += GMPC_THREADS) {
        const bool isx = e < Nx;
        const int j = isx ? e : e - Nx;
        const int K = isx ? Kx : Ku, N = isx ? Nx : Nu;
        const float* W = isx ? net.hx.W[l] : net.hu.W[l];
        const float* in = isx ? inx : inu;
        float acc = (isx ? net.hx.b[l] : net.hu.b[l])[j];
        for (int k = 0; k < K; ++k) acc = fmaf(in[k], W[(size_t)k * N + j], acc);
        if (l < L - 1) {
          acc = fmaxf(acc, 0.f);
          if (a.grad) arow[(isx ? net.ax[l + 1] : net.au[l + 1]) + j] = acc;
        }
        out[(isx ? 0 : hw) + j] = acc;
      }
      __syncthreads();
      inx = out;
      inu = out + hw;
      float* sw = out; out = other; other = sw;
    }
    // ---- outputs, loss; next_x becomes the next input (own elements only)
    for (int e = tid; e < n + m; e += GMPC_THREADS) {
      float v, ref;
      if (e < n) {
        v = inx[e] + xin[e];
        ref = a.yseq[row * n + e];
        xin[e] = v;
      } else {
        v = tanhf(inu[e - n]);
        ref = a.useq[row * m + e - n];
      }
      if (a.grad) sv[so + e] = v;
      const float df = v - ref;
      lsum = fmaf(disc * df, df, lsum);
    }
    disc *= a.gamma;
    __syncthreads();
  }
  lsum = efit_block_sum(lsum, red);
  if (tid == 0) a.loss[b] = lsum;
  if (!a.grad) return;
  // ---------------------------------------------------------------- BPTT
  for (int i = tid; i < n; i += GMPC_THREADS) lam[i] = 0.f;
  for (int j = tid; j < F; j += GMPC_THREADS) { dhv[j] = 0.f; dcv[j] = 0.f; }
  __syncthreads();
  for (int t = S - 1; t >= 0; --t) {
    const size_t row = (size_t)b * S + t;
    const float* arow = a.acts + row * net.stride;
    float* drow = a.dels + row * net.stride;
    const float* sv = a.save + row * a.sstride;
    float dt = 1.f;
    for (int k = 0; k < t; ++k) dt *= a.gamma;    // the forward's discount, bit for bit
    // deltas at the heads' outputs: 2 g^t (next_x - y) + lam (kept in lam for the residual path), and
    // 2 g^t (u - a) tanh'
    for (int e = tid; e < n + m; e += GMPC_THREADS) {
      if (e < n) {
        const float g = 2.f * dt * (sv[so + e] - a.yseq[row * n + e]) + lam[e];
        lam[e] = g;
        hA[e] = g;
        drow[net.dx[L - 1] + e] = g;
      } else {
        const int j = e - n;
        const float u = sv[so + e];
        const float g = 2.f * dt * (u - a.useq[row * m + j]) * (1.f - u * u);
        hA[hw + j] = g;
        drow[net.du[L - 1] + j] = g;
      }
    }
    __syncthreads();
    float* cur = hA;
    float* nxt = hB;
    for (int l = L - 1; l >= 1; --l) {
      const int Kx = net.hx.dims[l], Nx = net.hx.dims[l + 1], Ku = net.hu.dims[l], Nu = net.hu.dims[l + 1];
      for (int e = tid; e < Kx + Ku; e += GMPC_THREADS) {
        const bool isx = e < Kx;
        const int k = isx ? e : e - Kx;
        const int N = isx ? Nx : Nu;
        const float* w = (isx ? net.hx.W[l] : net.hu.W[l]) + (size_t)k * N;
        const float* d = cur + (isx ? 0 : hw);
        float acc = 0.f;
        for (int j = 0; j < N; ++j) acc = fmaf(w[j], d[j], acc);
        acc = arow[(isx ? net.ax[l] : net.au[l]) + k] > 0.f ? acc : 0.f;    // relu'(a_l)
        nxt[(isx ? 0 : hw) + k] = acc;
        drow[(isx ? net.dx[l - 1] : net.du[l - 1]) + k] = acc;
      }
      __syncthreads();
      float* sw = cur; cur = nxt; nxt = sw;
    }
    // d loss / d y: both heads' first layers
    {
      const int Nx = net.hx.dims[1], Nu = net.hu.dims[1];
      for (int k = tid; k < Y; k += GMPC_THREADS) {
        const float* wx = net.hx.W[0] + (size_t)k * Nx;
        const float* wu = net.hu.W[0] + (size_t)k * Nu;
        float accx = 0.f, accu = 0.f;
        for (int j = 0; j < Nx; ++j) accx = fmaf(wx[j], cur[j], accx);
        for (int j = 0; j < Nu; ++j) accu = fmaf(wu[j], cur[hw + j], accu);
        const float dy = accx + accu;
        if (F > 0) {
          yv[k] = dy;
        } else {
          const float dz = arow[ay + k] > 0.f ? dy : 0.f;
          zg[k] = dz;
          drow[k] = dz;
        }
      }
    }
    __syncthreads();
    if (F > 0) {
      for (int j = tid; j < F; j += GMPC_THREADS) {
        const float ig = sv[j], fg = sv[F + j], gg = sv[2 * F + j], og = sv[3 * F + j];
        const float cp = sv[G4 + j], tc = sv[5 * F + j];
        const float dh2 = yv[j] + dhv[j];
        const float dc2 = dcv[j] + dh2 * og * (1.f - tc * tc);
        const float dzi = dc2 * gg * ig * (1.f - ig), dzf = dc2 * cp * fg * (1.f - fg);
        const float dzg = dc2 * ig * (1.f - gg * gg), dzo = dh2 * tc * og * (1.f - og);
        zg[j] = dzi; zg[F + j] = dzf; zg[2 * F + j] = dzg; zg[3 * F + j] = dzo;
        drow[j] = dzi; drow[F + j] = dzf; drow[2 * F + j] = dzg; drow[3 * F + j] = dzo;
        dcv[j] = dc2 * fg;
      }
      __syncthreads();
      for (int k = tid; k < F; k += GMPC_THREADS) {
        const float* w = net.Wcat + (size_t)(n + k) * G4;
        float acc = 0.f;
        for (int j = 0; j < G4; ++j) acc = fmaf(w[j], zg[j], acc);
        dhv[k] = acc;
      }
    }
    // d x_in = W_first dz + (residual) the state head's output delta; it reaches next_x_{t-1} only when
    // the input was that prediction
    for (int i = tid; i < n; i += GMPC_THREADS) {
      float acc = 0.f;
      if (!a.teacher_forcing && t > 0) {
        const float* w = net.Wcat + (size_t)i * G;
        for (int j = 0; j < G; ++j) acc = fmaf(w[j], zg[j], acc);
        acc += lam[i];
      }
      lam[i] = acc;
    }
    __syncthreads();
  }
}

void gmpc_launch_expert_fit(const ExpertFitArgs& a, hipStream_t s) {
  const ExpertNet& e = a.net;
  const int G = e.F > 0 ? 4 * e.F : e.Y;
  const size_t lds = ((size_t)2 * e.n + 4 * (size_t)e.F + G + e.Y + 4 * (size_t)e.hw) * sizeof(float);
  hipLaunchKernelGGL(k_expert_fit, dim3(a.B), dim3(GMPC_THREADS), lds, s, a);
}
