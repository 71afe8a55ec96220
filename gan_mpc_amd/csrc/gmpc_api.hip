// C-ABI entry points of libgan_mpc_amd.so (include/gan_mpc_amd.h): errors, shapes, the context's life, parameter
// layouts, profile and debug accessors.  gmpc_api_{solve,sampled,critic,grads}.hip hold the rest.
#include <cstdarg>
#include <new>

#include "gmpc_ctx.h"
#include "gmpc_fused_solve.h"

// error handling -------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
int gmpc_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

extern "C" const char* gmpc_last_error(void) { return g_err; }
extern "C" const char* gmpc_version(void) { return "gan_mpc_amd 0.1 (gfx950)"; }

static int check_shape(const gmpc_shape* s) {
  if (!s) return fail(GMPC_EINVAL, "shape is null");
  if (s->n < 1 || s->m < 1 || s->T < 1) return fail(GMPC_EINVAL, "n, m, T must be positive");
  if (s->n > 1024 || s->m > 64)
    return fail(GMPC_EINVAL, "unsupported shape n=%d m=%d: n <= 1024 and m <= 64 are built", s->n, s->m);
  // (n <= 64 with more than 32 controls: the fused small-state kernels hold an m x m factor per lane and the gain
  // block of a step in LDS; such shapes take the step-major pipeline of the large-state path, which is general)
  if (s->dyn_layers < 1 || s->dyn_layers > GMPC_MAX_LAYERS)
    return fail(GMPC_EINVAL, "dyn_layers must be in [2, %d]", GMPC_MAX_LAYERS);
  if (s->cost_layers < 1 || s->cost_layers > GMPC_MAX_LAYERS)
    return fail(GMPC_EINVAL, "cost_layers must be in [1, %d]", GMPC_MAX_LAYERS);
  if (s->dyn_lstm_features > 0) {
    // LSTM dynamics variant: xc = [x, c, h], dyn_dims describes the relu tail h' -> x
    const int Fd = s->dyn_lstm_features, nx = s->x_size;
    if (Fd > 128) return fail(GMPC_EINVAL, "unsupported shape: dynamics lstm_features = %d > 128", Fd);
    if (nx < 1 || s->n != nx + 2 * Fd)
      return fail(GMPC_EINVAL, "LSTM dynamics: n must be x_size + 2 * dyn_lstm_features (n=%d, x_size=%d, F=%d)",
                  s->n, nx, Fd);
    if (s->dyn_dims[0] != Fd || s->dyn_dims[s->dyn_layers] != nx)
      return fail(GMPC_EINVAL, "LSTM dynamics: dyn_dims (the tail) must start with dyn_lstm_features and end with x_size");
    if (s->dyn_layers < 1) return fail(GMPC_EINVAL, "dyn_layers must be >= 1");
  } else {
    if (s->x_size != 0 && s->x_size != s->n)
      return fail(GMPC_EINVAL, "x_size must equal n (or 0) for the MLP dynamics: its carry is empty");
    if (s->dyn_layers < 2)
      return fail(GMPC_EINVAL, "dyn_layers must be in [2, %d]", GMPC_MAX_LAYERS);
    if (s->dyn_dims[0] != s->n + s->m || s->dyn_dims[s->dyn_layers] != s->n)
      return fail(GMPC_EINVAL, "dyn_dims must start with n+m and end with n");
  }
  if (s->cost_dims[0] != s->n) return fail(GMPC_EINVAL, "cost_dims must start with n");
  if (s->cost_dims[s->cost_layers] > 32)
    return fail(GMPC_EINVAL, "cost fout must be <= 32");
  for (int l = 1; l < s->dyn_layers; ++l)
    if (s->dyn_dims[l] < 1 || s->dyn_dims[l] > GMPC_THREADS)
      return fail(GMPC_EINVAL, "dynamics hidden width must be in [1, %d]", GMPC_THREADS);
  for (int l = 1; l < s->cost_layers; ++l)
    if (s->cost_dims[l] < 1 || s->cost_dims[l] > GMPC_THREADS)
      return fail(GMPC_EINVAL, "cost hidden width must be in [1, %d]", GMPC_THREADS);
  if (s->lstm_features != 0) {
    // (64: gmpc_critic_lstm.hip's kernels and k_lstm_fwd / _bwd of gmpc_critic.hip; other counts: k_lstm_fwd_g / _bwd_g)
    if (s->lstm_features < 1 || s->lstm_features > 128)
      return fail(GMPC_EINVAL, "unsupported shape: critic lstm_features = %d outside [1, 128]", s->lstm_features);
    if (s->head_layers < 1 || s->head_layers > GMPC_MAX_LAYERS)
      return fail(GMPC_EINVAL, "head_layers must be in [1, %d]", GMPC_MAX_LAYERS);
    if (s->head_dims[0] != s->lstm_features || s->head_dims[s->head_layers] != 1)
      return fail(GMPC_EINVAL, "head_dims must start with F and end with 1");
    for (int l = 1; l < s->head_layers; ++l)
      if (s->head_dims[l] < 1 || s->head_dims[l] > GMPC_THREADS)
        return fail(GMPC_EINVAL, "head hidden width must be in [1, %d]", GMPC_THREADS);
  }
  return 0;
}

extern "C" long gmpc_param_count(const gmpc_shape* s, int which) {
  if (!s) return -1;
  if (which == 0) {
    const long Fd = s->dyn_lstm_features;
    const long cell = Fd > 0 ? ((long)s->x_size + s->m + Fd) * 4 * Fd + 4 * Fd : 0;
    return cell + mlp_count(s->dyn_layers, s->dyn_dims);
  }
  if (which == 1) return mlp_count(s->cost_layers, s->cost_dims);
  if (which == 2) {
    const long F = s->lstm_features;
    const long nx = s->x_size > 0 ? s->x_size : s->n;     // the critic scores x sequences
    return nx * 4 * F + F * 4 * F + 4 * F + mlp_count(s->head_layers, s->head_dims);
  }
  return -1;
}

static void transpose_mlp(const MlpDesc& d, hipStream_t s) {
  for (int l = 0; l < d.L; ++l)
    gmpc_launch_transpose(d.dims[l], d.dims[l + 1], d.W[l], const_cast<float*>(d.WT[l]), s);
}

extern "C" int gmpc_create(const gmpc_shape* shape, int max_batch, int device, gmpc_ctx** out) {
  if (!out) return fail(GMPC_EINVAL, "out is null");
  *out = nullptr;
  TRY(check_shape(shape));
  if (max_batch < 1) return fail(GMPC_EINVAL, "max_batch must be positive");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(GMPC_ENODEV, "no HIP device is visible; libgan_mpc_amd has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(GMPC_EINVAL, "device %d out of range", device);
  HIP_TRY(hipSetDevice(device));
  gmpc_ctx* c = new (std::nothrow) gmpc_ctx();
  if (!c) return fail(GMPC_ENOMEM, "out of host memory");
  c->sh = *shape;
  c->maxB = max_batch;
  c->device = device;
  if (hipDeviceGetAttribute(&c->ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) c->ncu = 256;
  const gmpc_shape& s = c->sh;
  const size_t B = max_batch, n = s.n, m = s.m, T = s.T, nm = n + m, Lh = s.dyn_layers - 1;
  c->dynl = s.dyn_lstm_features > 0;
  c->nx = c->dynl ? s.x_size : s.n;
  int rc = 0;
#define A_(p, cnt) if (!rc) rc = dalloc(c, &c->p, (cnt))
  A_(dynT, mlp_count(s.dyn_layers, s.dyn_dims));
  A_(costT, mlp_count(s.cost_layers, s.cost_dims));
  c->linpad_floats = c->dynl ? 0 : gmpc_linpad_floats(&c->sh);
  A_(linpad, c->linpad_floats);
  A_(masks, B * T * Lh * GMPC_MW);
  // line-search candidates: GMPC_LS_ITEMS per trajectory
  A_(maskc, GMPC_LS_ITEMS * B * T * Lh * GMPC_MW);
  A_(Xc, GMPC_LS_ITEMS * B * (T + 1) * n);
  A_(Uc, GMPC_LS_ITEMS * B * T * m);
  for (int i = 0; i < 2; ++i) {
    if (!rc) rc = dalloc(c, &c->lsw.item_b[i], GMPC_LS_ITEMS * B);
    if (!rc) rc = dalloc(c, &c->lsw.item_k[i], GMPC_LS_ITEMS * B);
  }
  if (!rc) rc = dalloc(c, &c->lsw.first, B);
  if (!rc) rc = dalloc(c, &c->lsw.slot, GMPC_LS_ITEMS * B);
  if (!rc) rc = dalloc(c, &c->lsw.cnt, B);
  if (!rc) rc = dalloc(c, &c->lsw.kfirst, B);
  if (!rc) rc = dalloc(c, &c->lsw.prevk, B);
  if (!rc) rc = dalloc(c, &c->lsw.counts, GMPC_LS_ROUNDS_MAX + 1 + GMPC_LS_STATS);
  if (!rc) rc = dalloc(c, &c->lsw.run, B);
  if (!rc) rc = dalloc(c, &c->lsw.objc, GMPC_LS_ITEMS * B);
  c->big = s.n > 64 || s.m > 32;
  if (!c->big) {
    A_(AB, B * T * n * nm);
  } else {
    // step-major backward pass: one step's Jacobians and the n x n work matrices, each followed by
    // zeroed rows the GEMMs may read past the end
    c->bw.n = s.n; c->bw.m = s.m; c->bw.T = s.T; c->bw.ng = c->nx;
    const size_t pad = 16 * nm;
#define B_(p, cnt) if (!rc) { rc = dalloc(c, &c->bw.p, (cnt)); if (!rc) (void)hipMemset(c->bw.p, 0, (cnt) * sizeof(float)); }
    B_(ABt, B * n * nm + pad);
    B_(P, B * n * n + pad);
    B_(PAB, B * n * nm + pad);
    B_(T1, B * n * n + pad);
    B_(HG, B * m * nm + pad);
    B_(KV, 2 * B * m * n + pad);
    B_(VK, 2 * B * m * n + pad);
    B_(pvec, B * n); B_(lam, B * n); B_(sbuf, B); B_(gn2, B);
    // low-rank form of the Jacobians (gmpc_large.hip): MLP dynamics whose last hidden width is below n / 2
    // (8 n^2 h instead of 4 n^3 flops per Riccati step); GMPC_BIG_DENSE=1 keeps the dense form (A/B timing)
    {
      const size_t hl = s.dyn_dims[s.dyn_layers - 1];
      size_t hmax = 0;
      for (int l = 1; l < s.dyn_layers; ++l) hmax = (size_t)s.dyn_dims[l] > hmax ? s.dyn_dims[l] : hmax;
      if (gmpc_big_lowrank_h(&c->sh) > 0) {
        c->bw.h = (int)hl;
        B_(Vt, B * hl * nm + pad);
        B_(W1b, B * hl * n + pad);
        B_(W2b, B * hl * nm + pad);
        B_(Sa, B * hmax * hl + pad);
        B_(Sb, B * hmax * hl + pad);
      }
    }
    // one-step-ahead Jacobians on a side stream (MLP dynamics, dense form)
    if (!c->dynl && c->bw.h == 0) {
      // (the second copy and the side stream are an optimisation: when any of them cannot be had -- the copy is
      // B n (n + m) floats, 4.5 GB at n = 1024 -- the pass runs on one stream with one buffer)
      if (!rc) {
        const size_t cnt2 = B * n * nm + pad;
        float* p2 = nullptr;
        bool ok = hipMalloc(reinterpret_cast<void**>(&p2), cnt2 * sizeof(float)) == hipSuccess;
        ok = ok && hipMemset(p2, 0, cnt2 * sizeof(float)) == hipSuccess;
        ok = ok && hipStreamCreateWithFlags(&c->bw.side, hipStreamNonBlocking) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&c->bw.ev_start, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; i < 2 && ok; ++i)
          ok = hipEventCreateWithFlags(&c->bw.ev_ready[i], hipEventDisableTiming) == hipSuccess &&
               hipEventCreateWithFlags(&c->bw.ev_free[i], hipEventDisableTiming) == hipSuccess;
        if (ok) {
          c->allocs.push_back(p2);
          c->bw.ABt2 = p2;
        } else {
          (void)hipGetLastError();
          if (p2) (void)hipFree(p2);
          if (c->bw.side) { (void)hipStreamDestroy(c->bw.side); c->bw.side = nullptr; }
          if (c->bw.ev_start) { (void)hipEventDestroy(c->bw.ev_start); c->bw.ev_start = nullptr; }
          for (int i = 0; i < 2; ++i) {
            if (c->bw.ev_ready[i]) { (void)hipEventDestroy(c->bw.ev_ready[i]); c->bw.ev_ready[i] = nullptr; }
            if (c->bw.ev_free[i]) { (void)hipEventDestroy(c->bw.ev_free[i]); c->bw.ev_free[i] = nullptr; }
          }
        }
      }
    }
#undef B_
    c->AB = c->bw.ABt;
  }
  A_(QT, B * n * n);
  A_(qT, B * n);
  A_(Xs, B * (T + 1) * n);
  A_(Us, B * T * m);
  A_(goals, B * (T + 1) * n);
  A_(Ks, B * T * m * n + 16 * nm);
  A_(ks, B * T * m);
  A_(grads, B * T * m);
  A_(adjs, B * (T + 1) * n);
  A_(obj, B); A_(alpha, B); A_(obj_step, B); A_(U_step, B);
  A_(iters, B); A_(cont, B);
  if (!c->dynl && !c->big && s.T <= GMPC_FZ_MAX_T) {
    A_(fzcand, B * GMPC_FZ_NC * ((T + 1) * n + T * m));
    A_(box_count, 2 * B);
    A_(box_iters, B * T);
    A_(box_clamped, B * T * m);
    A_(box_mask, B * T);
  }
  // bilevel
  c->drows = mlp_rows(s.dyn_layers, s.dyn_dims);
  c->crows = mlp_rows(s.cost_layers, s.cost_dims);
  A_(lx, B * (T + 1) * n);
  A_(Bvec, B * T * m);
  A_(Hout, B * T * m);
  A_(dX, B * (T + 1) * n);
  A_(gmpc, B * 3);
  A_(cact, (2 * B + GMPC_WGRAD_PAD) * c->crows.stride);
  A_(cdel, (2 * B + GMPC_WGRAD_PAD) * c->crows.stride);
  A_(bl_loss, B);
  // critic
  long wmax = 0;
  for (int l = 0; l < s.cost_layers; ++l) {
    long w = (long)s.cost_dims[l] * s.cost_dims[l + 1] + s.cost_dims[l + 1];
    if (w > wmax) wmax = w;
  }
  if (c->dynl) {
    A_(xg, B * (T + 1) * c->nx);
    A_(lxg, B * (T + 1) * c->nx);
    if (c->big) {
      if (!rc) rc = dalloc(c, &c->bw.Phi, B * nm * nm);
    } else {
      A_(phi, B * T * nm * nm);
    }
  }
  if (s.lstm_features > 0) {
    // (the saves of the LSTM kernels are laid out per workgroup of 4 sequences: round the batch up)
    const size_t Bc = (2 * B + 3) / 4 * 4, F = s.lstm_features, T1 = T + 1, n = c->nx;   // the critic scores x sequences
    c->hrows = mlp_rows(s.head_layers, s.head_dims);
    A_(critT, (n + F) * 4 * F + mlp_count(s.head_layers, s.head_dims));
    A_(gates, Bc * T1 * 4 * F);
    A_(cs, Bc * T1 * F);
    A_(hp, Bc * T1 * F);
    A_(hT, Bc * F);
    A_(dz, (Bc * T1 + GMPC_WGRAD_PAD) * 4 * F);
    if (n + F > GMPC_THREADS) {
      A_(WhT, 4 * F * F);
      A_(xT, Bc * T1 * n + 16 * Bc * T1);
      A_(xproj, (Bc * T1 + 16) * 4 * F);
    }
    {
      CriticDesc probe{};
      probe.n = (int)n; probe.F = (int)F; probe.T1 = (int)T1;
      if (gmpc_lstm2_supported(probe)) A_(lwp, gmpc_lstm2_wpart_floats(probe, (int)Bc));
    }
    A_(plast, (Bc + GMPC_WGRAD_PAD) * GMPC_HEAD2_LD);
    A_(hacts, (Bc + GMPC_WGRAD_PAD) * c->hrows.stride);
    A_(hdels, (Bc + GMPC_WGRAD_PAD) * c->hrows.stride);
    A_(dhT, Bc * F);
    A_(cscore, Bc);
    A_(closs, Bc);
    long w = (long)F * 4 * F + 4 * F;
    if (w > wmax) wmax = w;
    for (int l = 0; l < s.head_layers; ++l) {
      w = (long)s.head_dims[l] * s.head_dims[l + 1] + s.head_dims[l + 1];
      if (w > wmax) wmax = w;
    }
  }
  c->wpart_floats = 256 * wmax;
  if (c->wpart_floats < (12L << 20)) c->wpart_floats = 12L << 20;
  A_(wpart, c->wpart_floats);
  A_(scratch, 1024);
#undef A_
  // operands of the weight-gradient GEMM: its pad rows must be finite (GMPC_WGRAD_PAD)
  if (!rc && c->cdel) (void)hipMemset(c->cdel, 0, (2 * B + GMPC_WGRAD_PAD) * c->crows.stride * sizeof(float));
  if (!rc && c->cact) (void)hipMemset(c->cact, 0, (2 * B + GMPC_WGRAD_PAD) * c->crows.stride * sizeof(float));
  if (!rc && s.lstm_features > 0) {
    (void)hipMemset(c->dz, 0, ((size_t)2 * B * (T + 1) + GMPC_WGRAD_PAD) * 4 * s.lstm_features * sizeof(float));
    (void)hipMemset(c->hdels, 0, ((size_t)2 * B + GMPC_WGRAD_PAD) * c->hrows.stride * sizeof(float));
    (void)hipMemset(c->hacts, 0, ((size_t)2 * B + GMPC_WGRAD_PAD) * c->hrows.stride * sizeof(float));
    (void)hipMemset(c->plast, 0, ((size_t)2 * B + GMPC_WGRAD_PAD) * GMPC_HEAD2_LD * sizeof(float));
  }
  if (!rc) (void)hipMemset(c->Ks, 0, (B * T * m * n + 16 * nm) * sizeof(float));
  if (rc) {
    gmpc_destroy(c);
    return rc;
  }
  *out = c;
  return 0;
}

extern "C" int gmpc_destroy(gmpc_ctx* c) {
  if (!c) return 0;
  gmpc_comm_destroy_impl(&c->comm);
  if (c->hcont) {
    (void)hipHostFree(c->hcont);
    for (int i = 0; i < GMPC_POLL_DEPTH; ++i) (void)hipEventDestroy(c->poll_ev[i]);
  }
  if (c->crit_side) (void)hipStreamDestroy(c->crit_side);
  if (c->crit_fork) (void)hipEventDestroy(c->crit_fork);
  if (c->crit_join) (void)hipEventDestroy(c->crit_join);
  if (c->crit_tr) (void)hipEventDestroy(c->crit_tr);
  if (c->bw.side) (void)hipStreamDestroy(c->bw.side);
  if (c->bw.ev_start) (void)hipEventDestroy(c->bw.ev_start);
  for (int i = 0; i < 2; ++i) {
    if (c->bw.ev_ready[i]) (void)hipEventDestroy(c->bw.ev_ready[i]);
    if (c->bw.ev_free[i]) (void)hipEventDestroy(c->bw.ev_free[i]);
  }
  for (void* p : c->allocs) (void)hipFree(p);
  delete c;
  return 0;
}

extern "C" int gmpc_set_params(gmpc_ctx* c, const float* mpc_w, const float* dyn, const float* cost,
                               void* stream) {
  if (!c || !mpc_w || !dyn || !cost) return fail(GMPC_EINVAL, "null argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipSetDevice(c->device));
  (void)hipGetLastError();   // clean slate (see check_call)
  c->mpc_w = mpc_w;
  c->solB = 0;   // a held solution belongs to the previous parameters
  c->gradB = 0;
  c->w16_stale = true;   // the bf16 images of the sampled rollouts: rebuilt by the next bf16-mode solve
  bind_mlp(c->cost, c->sh.cost_layers, c->sh.cost_dims, cost, c->costT);
  transpose_mlp(c->cost, s);
  if (c->dynl) {
    // LSTM variant: Wx [(nx+m)][4F] | Wh [F][4F] | b [4F] | the tail's Dense layers
    const long Fd = c->sh.dyn_lstm_features, nx = c->nx, m = c->sh.m;
    c->dl.nx = (int)nx; c->dl.F = (int)Fd; c->dl.m = (int)m;
    c->dl.Wx = dyn;
    c->dl.Wh = dyn + (nx + m) * 4 * Fd;
    c->dl.b = c->dl.Wh + Fd * 4 * Fd;
    bind_mlp(c->dl.tail, c->sh.dyn_layers, c->sh.dyn_dims, c->dl.b + 4 * Fd, nullptr);
    c->dyn = c->dl.tail;     // generic fields (layer count for the mask bookkeeping of the line search)
  } else {
    bind_mlp(c->dyn, c->sh.dyn_layers, c->sh.dyn_dims, dyn, c->dynT);
    transpose_mlp(c->dyn, s);
    gmpc_linpad_prepare(c->dyn, c->sh.n, c->sh.m, c->linpad, c->linpad_floats, &c->lp, s);
  }
  if (getenv("GMPC_LIN_STAMPS")) {   // diagnostic build of the timing only; never set in production
    (void)hipMemsetAsync(c->scratch + 768, 0, 64, s);
    c->lp.dbg = reinterpret_cast<unsigned long long*>(c->scratch + 768);
  }
  HIP_TRY(hipGetLastError());
  c->params_set = true;
  return 0;
}

int check_call(gmpc_ctx* c, int B, bool need_params) {
  if (!c) return fail(GMPC_EINVAL, "ctx is null");
  if (need_params && !c->params_set) return fail(GMPC_EINVAL, "gmpc_set_params has not been called");
  if (B < 1 || B > c->maxB) return fail(GMPC_EINVAL, "B=%d outside [1, max_batch=%d]", B, c->maxB);
  if (hipSetDevice(c->device) != hipSuccess) return fail(GMPC_EHIP, "hipSetDevice failed");
  // hipGetLastError() is per-thread and shared with every other HIP user of the process (torch
  // leaves benign errors behind): start every entry point from a clean slate so that the checks
  // after our launches report only our own failures
  (void)hipGetLastError();
  return 0;
}

int GrowBuf::grow(gmpc_ctx* c, size_t floats) {
  if (cap >= floats) return 0;
  if (p) {
    for (size_t i = 0; i < c->allocs.size(); ++i)
      if (c->allocs[i] == p) { c->allocs.erase(c->allocs.begin() + i); break; }
    HIP_TRY(hipFree(p));
    p = nullptr;
    cap = 0;
  }
  TRY(dalloc(c, &p, floats));
  cap = floats;
  return 0;
}

int PadRows::reserve(gmpc_ctx* c, size_t rows, size_t stride, hipStream_t s) {
  TRY(grow(c, (rows + GMPC_WGRAD_PAD) * stride));
  HIP_TRY(hipMemsetAsync(p + rows * stride, 0, GMPC_WGRAD_PAD * stride * sizeof(float), s));
  return 0;
}

// flat parameter layouts, leaf by leaf (flax naming; see params.py of the host package)
static int add_leaf(gmpc_leaf* out, int max_leaves, int& k, const char* name, long off, int rows, int cols,
                    int ld) {
  if (out && k < max_leaves) {
    snprintf(out[k].name, sizeof(out[k].name), "%s", name);
    out[k].offset = off; out[k].rows = rows; out[k].cols = cols; out[k].ld = ld;
  }
  ++k;
  return 0;
}

static long mlp_leaves(gmpc_leaf* out, int max_leaves, int& k, const char* prefix, int L, const int* dims,
                       long off) {
  char nm[64];
  for (int l = 0; l < L; ++l) {
    snprintf(nm, sizeof(nm), "%sparams/Dense_%d/kernel", prefix, l);
    add_leaf(out, max_leaves, k, nm, off, dims[l], dims[l + 1], dims[l + 1]);
    off += (long)dims[l] * dims[l + 1];
    snprintf(nm, sizeof(nm), "%sparams/Dense_%d/bias", prefix, l);
    add_leaf(out, max_leaves, k, nm, off, 1, dims[l + 1], dims[l + 1]);
    off += dims[l + 1];
  }
  return off;
}

// an OptimizedLSTMCell's leaves: Wx [kin][4F], Wh [F][4F], b [4F]; flax' per-gate kernels are the column
// blocks g*F .. (g+1)*F
static long cell_leaves(gmpc_leaf* out, int max_leaves, int& k, const char* prefix, const char* scope, int kin,
                        int F, long off) {
  static const char gate[4] = {'i', 'f', 'g', 'o'};
  char nm[64];
  for (int g = 0; g < 4; ++g) {
    snprintf(nm, sizeof(nm), "%sparams/%s/i%c/kernel", prefix, scope, gate[g]);
    add_leaf(out, max_leaves, k, nm, off + (long)g * F, kin, F, 4 * F);
  }
  off += (long)kin * 4 * F;
  for (int g = 0; g < 4; ++g) {
    snprintf(nm, sizeof(nm), "%sparams/%s/h%c/kernel", prefix, scope, gate[g]);
    add_leaf(out, max_leaves, k, nm, off + (long)g * F, F, F, 4 * F);
  }
  off += (long)F * 4 * F;
  for (int g = 0; g < 4; ++g) {
    snprintf(nm, sizeof(nm), "%sparams/%s/h%c/bias", prefix, scope, gate[g]);
    add_leaf(out, max_leaves, k, nm, off + (long)g * F, 1, F, F);
  }
  return off + 4 * F;
}

static long critic_leaves(gmpc_leaf* out, int max_leaves, int& k, const char* prefix, const gmpc_shape* s,
                          long off) {
  const int nx = s->x_size > 0 ? s->x_size : s->n;
  off = cell_leaves(out, max_leaves, k, prefix, "ScanOptimizedLSTMCell_0", nx, s->lstm_features, off);
  return mlp_leaves(out, max_leaves, k, prefix, s->head_layers, s->head_dims, off);
}

static long dyn_leaves(gmpc_leaf* out, int max_leaves, int& k, const char* prefix, const gmpc_shape* s,
                       long off) {
  if (s->dyn_lstm_features > 0)
    off = cell_leaves(out, max_leaves, k, prefix, "OptimizedLSTMCell_0", s->x_size + s->m,
                      s->dyn_lstm_features, off);
  return mlp_leaves(out, max_leaves, k, prefix, s->dyn_layers, s->dyn_dims, off);
}

extern "C" int gmpc_pack_layout(const gmpc_shape* s, int which, gmpc_leaf* leaves, int max_leaves) {
  TRY(check_shape(s));
  if (max_leaves < 0 || (max_leaves > 0 && !leaves)) return fail(GMPC_EINVAL, "bad leaf buffer");
  int k = 0;
  switch (which) {
    case 0: dyn_leaves(leaves, max_leaves, k, "", s, 0); break;
    case 1: mlp_leaves(leaves, max_leaves, k, "", s->cost_layers, s->cost_dims, 0); break;
    case 2:
      if (s->lstm_features <= 0) return fail(GMPC_EINVAL, "this shape has no critic");
      critic_leaves(leaves, max_leaves, k, "", s, 0);
      break;
    case 3: {
      // the training vector of the host package: [mpc_weights | cost | dynamics | critic], so that the
      // trainable ranges of the reference's optimisers (gan/runner.py:51-63) are contiguous
      add_leaf(leaves, max_leaves, k, "mpc_weights", 0, 1, 3, 3);
      long off = mlp_leaves(leaves, max_leaves, k, "cost_params/", s->cost_layers, s->cost_dims, 3);
      off = dyn_leaves(leaves, max_leaves, k, "dynamics_params/", s, off);
      if (s->lstm_features > 0) critic_leaves(leaves, max_leaves, k, "critic_params/", s, off);
      break;
    }
    default: return fail(GMPC_EINVAL, "which must be 0 (dyn), 1 (cost), 2 (critic) or 3 (training vector)");
  }
  return k;
}

extern "C" int gmpc_set_linearize_event(gmpc_ctx* c, void* ev) {
  if (!c) return fail(GMPC_EINVAL, "ctx is null");
  c->lin_event = static_cast<hipEvent_t>(ev);
  return 0;
}

void set_lin_kernel(gmpc_ctx* c, int family) {
  switch (family) {
    case LIN_DYNL: c->lin_kernel = "k_dynl_jac"; break;
    case LIN_SPARSE:
      c->lin_kernel = c->sh.n > 16 ? "k_linearize_sparse (rows 0..15 per sample, rows 16..n-1 per time group)"
                                   : "k_linearize_sparse";
      break;
    case LIN_REGS:
      snprintf(c->lin_kernel_buf, sizeof(c->lin_kernel_buf), "%s", gmpc_linearize_regs_last_name());
      c->lin_kernel = c->lin_kernel_buf;
      break;
    case LIN_MFMA: c->lin_kernel = "k_linearize_mfma"; break;
    case LIN_VALU: c->lin_kernel = "k_linearize (vector ALU)"; break;
    case LIN_LOWRANK: c->lin_kernel = "low-rank factors (k_mask_scale, k_bgemm_tn)"; break;
    default: break;
  }
}

// The Jacobian chain a ctx of `shape` runs for nsamp samples (strided != 0: a strided sample set, as the large-state
// pass takes one time step of every trajectory), and the plan of k_linearize_mfma for it; host only.
extern "C" int gmpc_linearize_route(const gmpc_shape* shape, int nsamp, int strided, int* route) {
  TRY(check_shape(shape));
  if (nsamp < 1 || !route) return fail(GMPC_EINVAL, "bad argument");
  const gmpc_shape& s = *shape;
  const bool dynl = s.dyn_lstm_features > 0, big = s.n > 64 || s.m > 32;
  for (int i = 0; i < GMPC_LIN_ROUTE_INTS; ++i) route[i] = 0;
  route[0] = gmpc_linearize_family_of(big, gmpc_big_lowrank_h(shape), dynl, nsamp, s.n, s.m, s.dyn_layers, s.dyn_dims,
                                      strided != 0);
  if (dynl) return 0;
  LinMfmaPlan p;
  const int rc = gmpc_linearize_mfma_plan(nsamp, s.n, s.m, s.dyn_layers, s.dyn_dims, &p);
  route[1] = p.NT; route[2] = p.NTF; route[3] = p.NGF; route[4] = p.stage_w1; route[5] = p.stage_wl;
  route[6] = p.body; route[7] = p.ntiles; route[8] = p.grid; route[9] = (int)p.lds; route[10] = p.nsmax;
  route[11] = rc == 0 ? 1 : 0;
  return 0;
}

// The chain of the ctx's shape on the caller's masks, into the caller's AB [nsamp][n][n + m], with the weights and
// padded operands of the last gmpc_set_params: what the backward passes launch, for tests/linearize_cases.py.
extern "C" int gmpc_linearize_ex(gmpc_ctx* c, int nsamp, const unsigned* masks, const int* active, float* AB,
                                 int samp_mul, int samp_add, void* stream) {
  if (!c || !masks || !AB || nsamp < 1 || samp_mul < 1 || samp_add < 0) return fail(GMPC_EINVAL, "bad argument");
  if (!c->params_set) return fail(GMPC_EINVAL, "gmpc_set_params has not been called");
  const gmpc_shape& sh = c->sh;
  const bool strided = !(samp_mul == 1 && samp_add == 0);
  const int fam = gmpc_linearize_family_of(c->big, c->bw.h, c->dynl, nsamp, sh.n, sh.m, sh.dyn_layers, sh.dyn_dims,
                                           strided);
  if (fam == LIN_DYNL || fam == LIN_LOWRANK)
    return fail(GMPC_EINVAL, "gmpc_linearize_ex: LSTM dynamics and the low-rank form keep no Jacobian chain");
  // (the sparse chain's time groups and the VALU chain take whole horizons)
  if ((fam == LIN_SPARSE || fam == LIN_VALU) && !strided && nsamp % sh.T != 0)
    return fail(GMPC_EINVAL, "gmpc_linearize_ex: nsamp must be a multiple of T for this shape's chain");
  HIP_TRY(hipSetDevice(c->device));
  (void)hipGetLastError();   // clean slate (see check_call)
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (gmpc_launch_linearize_family(fam, nsamp, sh.T, sh.n, sh.m, c->dyn, c->lp, masks, active, AB, samp_mul, samp_add,
                                   s) != 0)
    return fail(GMPC_EINVAL, "gmpc_linearize_ex: no Jacobian chain covers this launch");
  set_lin_kernel(c, fam);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int gmpc_profile_enable(gmpc_ctx* c, int on) {
  if (!c) return fail(GMPC_EINVAL, "ctx is null");
  c->prof = on != 0;
  return 0;
}

extern "C" const char* gmpc_profile_kernel_name(gmpc_ctx* c, int slot) {
  if (!c || slot != PROF_LINEARIZE) return "";
  return c->lin_kernel;
}

extern "C" int gmpc_profile_read(gmpc_ctx* c, int slot, double* total_ms, int* count) {
  if (!c || slot < 0 || slot >= GMPC_PROF_SLOTS || !total_ms || !count)
    return fail(GMPC_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  (void)hipGetLastError();   // clean slate (see check_call)
  double tot = 0.0;
  int n = 0;
  for (auto& pr : c->prof_ev[slot]) {
    HIP_TRY(hipEventSynchronize(pr.second));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, pr.first, pr.second));
    tot += ms;
    ++n;
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  c->prof_ev[slot].clear();
  *total_ms = tot;
  *count = n;
  return 0;
}

// accessors used by the bilevel parity tests and the Python mirror (device pointers, valid until the
// next solve): 0 X, 1 U, 2 H (A^-1 B), 3 dX, 4 Bvec, 5 AB, 6 K, 7 k; of gmpc_ilqr_solve_box (null on shapes it does not
// cover): 15 [B][2] QPs that hit the iteration cap / QP iterations of the solve, 16 [B][T] QP iterations and 17
// [B][T][m] clamped flags of the last backward pass; of gmpc_ilqr_solve_box_held: 18 [B][T] 32-bit words (read them as
// such), bit j = control j is in the clamped set the bilevel tail differentiates through
extern "C" long gmpc_debug_buffer_count(gmpc_ctx* c, int which) {
  if (!c) return 0;
  const gmpc_shape& s = c->sh;
  const long B = c->maxB, n = s.n, m = s.m, T = s.T;
  switch (which) {
    case 0: case 3: return B * (T + 1) * n;
    case 1: case 2: case 4: case 7: return B * T * m;
    case 5: return c->big ? B * n * (n + m) : B * T * n * (n + m);
    case 6: return B * T * m * n;
    case 8: case 9: case 10: return B;
    case 11: return B * (T + 1) * n;
    case 12: return (long)GMPC_LS_ITEMS * B * (T + 1) * n;
    case 13: return (long)GMPC_LS_ITEMS * B * T * m;
    case 14: return 256;
    case 15: return c->box_count ? 2 * B : 0;
    case 16: return c->box_iters ? B * T : 0;
    case 17: return c->box_clamped ? B * T * m : 0;
    case 18: return c->box_mask ? B * T : 0;
    default: return 0;
  }
}

extern "C" const float* gmpc_debug_buffer(gmpc_ctx* c, int which) {
  if (!c) return nullptr;
  switch (which) {
    case 0: return c->Xs; case 1: return c->Us; case 2: return c->Hout; case 3: return c->dX;
    case 4: return c->Bvec; case 5: return c->AB; case 6: return c->Ks; case 7: return c->ks;
    case 14: return c->scratch + 768; case 12: return c->Xc; case 13: return c->Uc;
    case 8: return c->alpha; case 9: return c->obj_step; case 10: return c->U_step;
    case 11: return c->lx;
    case 15: return c->box_count; case 16: return c->box_iters; case 17: return c->box_clamped;
    case 18: return reinterpret_cast<const float*>(c->box_mask);
    default: return nullptr;
  }
}
