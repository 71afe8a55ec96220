// The VJP of the expert sequence model's rollout (gmpc_expert.hip: k_expert_seq) for caller cotangents
// g_goal = dL/dgoal [B][T+1][n] and g_U = dL/dinit_U [B][T][m]: dL/d(expert parameters) summed over the batch and
// dL/dhistory per window.
//
// The schedule is the rollout's: steps st = 0 .. hist + T - 1, the input of step st is history[st] for st <= hist and
// the previous step's next_x after that; goal[st - hist + 1] = next_x_st and init_U[st - hist] = u_st for st >= hist,
// goal[0] = history[hist].  So, in reverse time:
//   - steps st >= hist have head deltas: d next_x_st = g_goal[st - hist + 1] + lam (lam: what step st + 1's input
//     carries back, residual included; it exists only for st + 1 > hist), d(head_u output) = g_U[st - hist] (1 - u^2);
//   - steps st < hist have none: they receive gradient through the LSTM carry alone.  The MLP variant has no carry, so
//     those steps contribute nothing: it starts at st = hist, and rows < hist of grad_history are zero;
//   - d x_in_st = W_first dz + (st >= hist) d next_x_st goes to lam for st > hist and to grad_history[st] otherwise;
//     g_goal[0] is added to grad_history[hist].
//
// k_expert_vjp: one 512-thread workgroup owns 4 windows as float4 components (k_expert_seq's form: one weight read
// serves four windows), runs the forward and then the reverse sweep.  Every matrix-vector product of either sweep is
// "thread j = output j" over a row-major operand, coalesced over j: the reverse sweep reads the transposed weight copies
// that k_transpose_all (gmpc_optim.hip) builds into the call workspace (one launch: [Wx; Wh] or W_first, and every head
// layer).
// The kernel keeps per (workgroup, step) a float4 save row [activated gates (4F) | c_prev (F) | tanh c' (F) | u (m)] and
// emits per (step, window) the row operands of the weight-gradient GEMMs in k_expert_fit's column layout
// (ExpertNet, bind_expert):
//   acts row: [x_in (n) | h_prev (F) | y (Y) | head_x inputs a_1..a_{L-1} | head_u inputs ...]   (the relu state too)
//   dels row: [dz (4F) or d y_pre (Y) | head_x output deltas d_1..d_L | head_u output deltas d_1..d_L]
// Rows are step-major, row = (st - st0) B + b with st0 = 0 (LSTM) or hist (MLP), so the rows with head deltas are the
// contiguous tail (st >= hist) and the heads' GEMMs run over those T B rows only.  No atomics: identical calls give
// identical bits.
#include "gmpc_launch.h"

#define GMPC_EV_THREADS 512

__global__ __launch_bounds__(GMPC_EV_THREADS) void k_expert_vjp(ExpertVjpArgs a) {
  constexpr int SB = 4;
  extern __shared__ __attribute__((aligned(16))) char smem_ev[];
  const ExpertNet& net = a.net;
  const int n = net.n, m = net.m, F = net.F, Y = net.Y, G4 = 4 * F, L = net.hx.L, hw = net.hw, B = a.B;
  float4* act = reinterpret_cast<float4*>(smem_ev);     // [n + F] forward: x | h;  reverse: lam | dh
  float4* gbuf = act + (n + F);                         // [4F or Y] gates (forward), first-layer delta (reverse)
  float4* hA = gbuf + (F > 0 ? G4 : Y);                 // [2 hw] x half | u half
  float4* hB = hA + 2 * hw;                             // [2 hw]
  float* actf = reinterpret_cast<float*>(act);
  float* gbf = reinterpret_cast<float*>(gbuf);
  const int tid = threadIdx.x;
  const int s0 = blockIdx.x * SB;
  const int half = tid >> 8, hj = tid & 255;            // head: 0 = state, 1 = action; neuron index
  const MlpDesc& hd = half == 0 ? net.hx : net.hu;
  const int* aoff = half == 0 ? net.ax : net.au;
  const int* doff = half == 0 ? net.dx : net.du;
  const int hist = a.hist, T = a.T, S = hist + T, st0 = a.st0;
  const int ay = n + F;                                 // acts offset of y
  const int su = F > 0 ? 6 * F : 0;                     // save offset of u
  const size_t stride = net.stride;
  // windows past B (the last workgroup) compute on window B - 1's data and write nothing
  int bw[SB];
  bool ok[SB];
#pragma unroll
  for (int cc = 0; cc < SB; ++cc) { bw[cc] = min(s0 + cc, B - 1); ok[cc] = s0 + cc < B; }
  float4* save = a.save + (size_t)blockIdx.x * (S - st0) * a.sstride;
  auto put = [&](float* rows, int st, int col, const float4& v) {
#pragma unroll
    for (int cc = 0; cc < SB; ++cc)
      if (ok[cc]) rows[((size_t)(st - st0) * B + bw[cc]) * stride + col] = f4get(v, cc);
  };
  auto get = [&](const float* rows, int st, int col) {
    float4 v;
#pragma unroll
    for (int cc = 0; cc < SB; ++cc) f4set(v, cc, rows[((size_t)(st - st0) * B + bw[cc]) * stride + col]);
    return v;
  };
  // ------------------------------------------------------------------------------------------- forward
  float c = 0.f;                                        // cell state of (unit tid % F, window tid / F)
  for (int e = tid; e < F * SB; e += GMPC_EV_THREADS) actf[n * SB + e] = 0.f;     // h = 0
  for (int st = st0; st < S; ++st) {
    float4* sv = save + (size_t)(st - st0) * a.sstride;
    float* svf = reinterpret_cast<float*>(sv);
    if (st <= hist) {
      for (int e = tid; e < n * SB; e += GMPC_EV_THREADS) {
        const int sb = e / n, i = e - sb * n;
        actf[i * SB + sb] = a.history[((size_t)min(s0 + sb, B - 1) * (hist + 1) + st) * n + i];
      }
    }
    __syncthreads();
    for (int j = tid; j < n + F; j += GMPC_EV_THREADS) put(a.acts, st, j, act[j]);
    if (F > 0) {
      if (tid < G4) {
        const float bj = net.bcat[tid];
        float4 acc[1] = {make_float4(bj, bj, bj, bj)};
        dense_rows<1>(net.Wcat, n + F, G4, tid, act, acc);
        float4 v = acc[0];
        if (tid >= 2 * F && tid < 3 * F) { v.x = tanhf(v.x); v.y = tanhf(v.y); v.z = tanhf(v.z); v.w = tanhf(v.w); }
        else { v.x = sigmoidf_(v.x); v.y = sigmoidf_(v.y); v.z = sigmoidf_(v.z); v.w = sigmoidf_(v.w); }
        gbuf[tid] = v;
        sv[tid] = v;
      }
      __syncthreads();
      if (tid < F * SB) {
        const int u = tid % F, sb = tid / F;
        const float ig = gbf[(0 * F + u) * SB + sb], fg = gbf[(1 * F + u) * SB + sb];
        const float gg = gbf[(2 * F + u) * SB + sb], og = gbf[(3 * F + u) * SB + sb];
        svf[(G4 + u) * SB + sb] = c;
        c = fg * c + ig * gg;
        const float tc = tanhf(c);
        svf[(5 * F + u) * SB + sb] = tc;
        actf[(n + u) * SB + sb] = og * tc;
      }
      __syncthreads();
      if (st < hist) continue;        // teacher-forced step: only the carry goes on (block-uniform)
      if (hj < F) hA[half * hw + hj] = act[n + hj];
      if (tid < F) put(a.acts, st, ay + tid, act[n + tid]);
    } else {
      if (tid < Y) {
        const float bj = net.bcat[tid];
        float4 acc[1] = {make_float4(bj, bj, bj, bj)};
        dense_rows<1>(net.Wcat, n, Y, tid, act, acc);
        const float4 v = make_float4(fmaxf(acc[0].x, 0.f), fmaxf(acc[0].y, 0.f), fmaxf(acc[0].z, 0.f),
                                     fmaxf(acc[0].w, 0.f));
        hA[tid] = v;
        hA[hw + tid] = v;
        put(a.acts, st, ay + tid, v);
      }
    }
    __syncthreads();
    // heads (same depth): state head on threads 0..255, action head on 256..511
    float4* in = hA;
    float4* out = hB;
    for (int l = 0; l < L; ++l) {
      const int K = hd.dims[l], N = hd.dims[l + 1];
      for (int j = hj; j < N; j += 256) {
        const float bj = hd.b[l][j];
        float4 acc[1] = {make_float4(bj, bj, bj, bj)};
        dense_rows<1>(hd.W[l], K, N, j, in + half * hw, acc);
        float4 v = acc[0];
        if (l < L - 1) {
          v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
          put(a.acts, st, aoff[l + 1] + j, v);
        }
        out[half * hw + j] = v;
      }
      __syncthreads();
      float4* tmp = in; in = out; out = tmp;
    }
    // next_x = head_x + x becomes the next input; u = tanh(head_u) is kept for its derivative
    if (half == 0) {
      for (int j = hj; j < n; j += 256) {
        const float4 x = act[j], o = in[j];
        act[j] = make_float4(o.x + x.x, o.y + x.y, o.z + x.z, o.w + x.w);
      }
    } else {
      for (int j = hj; j < m; j += 256) {
        const float4 o = in[hw + j];
        sv[su + j] = make_float4(tanhf(o.x), tanhf(o.y), tanhf(o.z), tanhf(o.w));
      }
    }
    __syncthreads();
  }
  // ------------------------------------------------------------------------------------------- reverse sweep
  for (int j = tid; j < n + F; j += GMPC_EV_THREADS) act[j] = make_float4(0.f, 0.f, 0.f, 0.f);   // lam = 0, dh = 0
  if (F == 0 && a.grad_history) {
    // no carry: the teacher-forced rows reach nothing
    for (int e = tid; e < hist * n; e += GMPC_EV_THREADS)
#pragma unroll
      for (int cc = 0; cc < SB; ++cc)
        if (ok[cc]) a.grad_history[(size_t)bw[cc] * (hist + 1) * n + e] = 0.f;
  }
  float dc = 0.f;                                       // d loss / d cell state of (unit tid % F, window tid / F)
  __syncthreads();
  for (int st = S - 1; st >= st0; --st) {
    const float4* sv = save + (size_t)(st - st0) * a.sstride;
    const float* svf = reinterpret_cast<const float*>(sv);
    const bool live = st >= hist;                       // a step with head deltas
    const int t = st - hist;
    float4* cur = hA;
    float4* nxt = hB;
    if (live) {
      // deltas at the heads' outputs: g_goal + lam (kept in lam for the residual path), g_U tanh'
      if (half == 0) {
        for (int j = hj; j < n; j += 256) {
          float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
          if (a.g_goal) {
#pragma unroll
            for (int cc = 0; cc < SB; ++cc) f4set(g, cc, a.g_goal[((size_t)bw[cc] * (T + 1) + t + 1) * n + j]);
          }
          const float4 lm = act[j];
          const float4 v = make_float4(g.x + lm.x, g.y + lm.y, g.z + lm.z, g.w + lm.w);
          act[j] = v;          // own element
          hA[j] = v;
          if (a.dels) put(a.dels, st, net.dx[L - 1] + j, v);
        }
      } else {
        for (int j = hj; j < m; j += 256) {
          float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
          if (a.g_U) {
#pragma unroll
            for (int cc = 0; cc < SB; ++cc) f4set(g, cc, a.g_U[((size_t)bw[cc] * T + t) * m + j]);
          }
          const float4 u = sv[su + j];
          const float4 v = make_float4(g.x * (1.f - u.x * u.x), g.y * (1.f - u.y * u.y), g.z * (1.f - u.z * u.z),
                                       g.w * (1.f - u.w * u.w));
          hA[hw + j] = v;
          if (a.dels) put(a.dels, st, net.du[L - 1] + j, v);
        }
      }
      __syncthreads();
      // back through the heads over the transposed copies: thread k = input unit k of layer l
      for (int l = L - 1; l >= 0; --l) {
        const int K = hd.dims[l], N = hd.dims[l + 1];
        for (int k = hj; k < K; k += 256) {
          float4 acc[1] = {make_float4(0.f, 0.f, 0.f, 0.f)};
          dense_rows<1>(hd.WT[l], N, K, k, cur + half * hw, acc);
          float4 v = acc[0];
          if (l >= 1) {
            const float4 al = get(a.acts, st, aoff[l] + k);                  // relu'(a_l)
            v.x = al.x > 0.f ? v.x : 0.f; v.y = al.y > 0.f ? v.y : 0.f;
            v.z = al.z > 0.f ? v.z : 0.f; v.w = al.w > 0.f ? v.w : 0.f;
            if (a.dels) put(a.dels, st, doff[l - 1] + k, v);
          }
          nxt[half * hw + k] = v;
        }
        __syncthreads();
        float4* sw = cur; cur = nxt; nxt = sw;
      }
    }
    // cur: the two heads' shares of d loss / d y (live steps)
    const bool need_x = st > hist || a.grad_history != nullptr;
    if (F > 0) {
      if (tid < F * SB) {
        const int u = tid % F, sb = tid / F;
        const float* curf = reinterpret_cast<const float*>(cur);
        const float ig = svf[(0 * F + u) * SB + sb], fg = svf[(1 * F + u) * SB + sb];
        const float gg = svf[(2 * F + u) * SB + sb], og = svf[(3 * F + u) * SB + sb];
        const float cp = svf[(G4 + u) * SB + sb], tc = svf[(5 * F + u) * SB + sb];
        const float dy = live ? curf[u * SB + sb] + curf[(hw + u) * SB + sb] : 0.f;
        const float dh2 = dy + actf[(n + u) * SB + sb];
        const float dc2 = dc + dh2 * og * (1.f - tc * tc);
        gbf[(0 * F + u) * SB + sb] = dc2 * gg * ig * (1.f - ig);
        gbf[(1 * F + u) * SB + sb] = dc2 * cp * fg * (1.f - fg);
        gbf[(2 * F + u) * SB + sb] = dc2 * ig * (1.f - gg * gg);
        gbf[(3 * F + u) * SB + sb] = dh2 * tc * og * (1.f - og);
        dc = dc2 * fg;
      }
      __syncthreads();
      if (a.dels && tid < G4) put(a.dels, st, tid, gbuf[tid]);
    } else {
      if (tid < Y) {
        const float4 y = get(a.acts, st, ay + tid);
        const float4 p = cur[tid], q = cur[hw + tid];
        const float4 v = make_float4(y.x > 0.f ? p.x + q.x : 0.f, y.y > 0.f ? p.y + q.y : 0.f,
                                     y.z > 0.f ? p.z + q.z : 0.f, y.w > 0.f ? p.w + q.w : 0.f);
        gbuf[tid] = v;
        if (a.dels) put(a.dels, st, tid, v);
      }
      __syncthreads();
    }
    // [d x_in | d h_prev] = [Wx; Wh] dz (or W_first dz): thread k = row k of the matrix, over its transposed copy
    const int KG = F > 0 ? G4 : Y;
    for (int k = (need_x ? 0 : n) + tid; k < n + F; k += GMPC_EV_THREADS) {
      float4 acc[1] = {make_float4(0.f, 0.f, 0.f, 0.f)};
      dense_rows<1>(net.WcatT, KG, n + F, k, gbuf, acc);
      float4 v = acc[0];
      if (k >= n) {
        act[k] = v;            // dh
      } else {
        if (live) {
          const float4 lm = act[k];                      // residual: next_x = head_x + x_in
          v = make_float4(v.x + lm.x, v.y + lm.y, v.z + lm.z, v.w + lm.w);
        }
        if (st > hist) {
          act[k] = v;          // the input was step st - 1's next_x
        } else {
#pragma unroll
          for (int cc = 0; cc < SB; ++cc) {
            float o = f4get(v, cc);
            if (st == hist && a.g_goal) o += a.g_goal[(size_t)bw[cc] * (T + 1) * n + k];   // goal[0] = history[hist]
            if (ok[cc]) a.grad_history[((size_t)bw[cc] * (hist + 1) + st) * n + k] = o;
          }
        }
      }
    }
    __syncthreads();
  }
}

size_t gmpc_expert_vjp_save_floats(const ExpertVjpArgs& a) {
  return (size_t)((a.B + 3) / 4) * (a.hist + a.T - a.st0) * a.sstride * 4;
}

int gmpc_launch_expert_vjp(const ExpertVjpArgs& a, hipStream_t s) {
  const ExpertNet& e = a.net;
  if (e.n > 1024 || e.m > 1024 || 4 * e.F > GMPC_EV_THREADS) return -1;
  if (e.hx.L != e.hu.L || e.hx.L < 1) return -1;
  if (e.F == 0 && e.Y > GMPC_EV_THREADS) return -1;      // MLP variant: one first-layer unit per thread
  const size_t lds = ((size_t)(e.n + e.F) + (e.F > 0 ? 4 * e.F : e.Y) + 4 * (size_t)e.hw) * sizeof(float4);
  if (lds > 159 * 1024) return -1;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_expert_vjp),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
    (void)hipGetLastError();
    attr = true;
  }
  // the transposed copies: [Wx; Wh] (or W_first) and every head layer, each at the matrix's own offset
  TransposeList mats{};
  auto add_mat = [&](int R, int C, const float* in, const float* out) {
    mats.R[mats.nm] = R; mats.C[mats.nm] = C; mats.in[mats.nm] = in; mats.out[mats.nm] = const_cast<float*>(out);
    ++mats.nm;
  };
  add_mat(e.n + e.F, e.F > 0 ? 4 * e.F : e.Y, e.Wcat, e.WcatT);
  for (int l = 0; l < e.hx.L; ++l) {
    add_mat(e.hx.dims[l], e.hx.dims[l + 1], e.hx.W[l], e.hx.WT[l]);
    add_mat(e.hu.dims[l], e.hu.dims[l + 1], e.hu.W[l], e.hu.WT[l]);
  }
  gmpc_launch_transpose_all(mats, s);
  hipLaunchKernelGGL(k_expert_vjp, dim3((a.B + 3) / 4), dim3(GMPC_EV_THREADS), lds, s, a);
  return 0;
}
