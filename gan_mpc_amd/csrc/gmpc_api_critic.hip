// C-ABI entry points of the critic and of what a training step does with gradients: the critic's loss / score, the
// upper-level loss, the Adam and Polyak steps, the batched GEMM's test entry, the multi-GPU exchange.
#include "gmpc_ctx.h"

// critic ---------------------------------------------------------------------------------------
static int bind_critic(gmpc_ctx* c, const float* critic, CriticDesc& cd, hipStream_t s, bool head_transpose = true) {
  const gmpc_shape& sh = c->sh;
  if (sh.lstm_features <= 0) return fail(GMPC_EINVAL, "this ctx was created without a critic");
  const long n = c->nx, F = sh.lstm_features;      // the critic scores x sequences
  cd.n = c->nx; cd.F = sh.lstm_features; cd.T1 = sh.T + 1;
  cd.Wcat = critic;
  cd.WcatT = c->critT;
  cd.b = critic + (n + F) * 4 * F;
  bind_mlp(cd.head, sh.head_layers, sh.head_dims, critic + (n + F) * 4 * F + 4 * F,
           c->critT + (n + F) * 4 * F);
  // the first-generation LSTM kernels read [Wx; Wh]^T; the second generation (n <= 32) and the head's forward
  // layers read the parameters as they lie, the head's backward layers its transposed kernels (one launch)
  if (!(c->lwp != nullptr && gmpc_lstm2_supported(cd)) || c->xT != nullptr)
    gmpc_launch_transpose((int)(n + F), (int)(4 * F), cd.Wcat, c->critT, s);
  if (head_transpose) gmpc_launch_mlp_transpose_all(cd.head, s);     // (else: the caller, beside the LSTM forward sweep)
  return 0;
}

static int critic_forward_backward(gmpc_ctx* c, int Bc, const float* xseq, const float* label,
                                   const float* critic, int loss_kind, float* dxseq, bool want_wgrad,
                                   float* grad_sum, hipStream_t s, float* loss_sum = nullptr) {
  // The side stream of the critic step (GMPC_CRITIC_SIDE=0: everything on the caller's stream): the transposed head
  // kernels are built beside the LSTM forward sweep (only k_head2 reads them), the head's weight gradients and the
  // loss sum run beside the BPTT sweep (they need k_head2's outputs only; the sweep is a latency chain at one wave
  // per SIMD).
  const char* side_env = getenv("GMPC_CRITIC_SIDE");
  const bool side_on = !(side_env != nullptr && side_env[0] == '0') && c->xT == nullptr && c->lwp != nullptr;
  if (side_on && !c->crit_side) {
    HIP_TRY(hipStreamCreateWithFlags(&c->crit_side, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&c->crit_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&c->crit_join, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&c->crit_tr, hipEventDisableTiming));
  }
  // (an error return between a fork onto the side stream and its join must not leave work in flight there)
  struct SideGuard {
    hipStream_t st = nullptr;
    ~SideGuard() { if (st) { (void)hipStreamSynchronize(st); (void)hipGetLastError(); } }
  } side_guard;
  CriticDesc cd;
  TRY(bind_critic(c, critic, cd, s, !side_on));
  const bool tr_side = side_on && gmpc_lstm2_supported(cd);
  if (side_on && !tr_side) gmpc_launch_mlp_transpose_all(cd.head, s);
  if (tr_side) {
    HIP_TRY(hipEventRecord(c->crit_fork, s));
    HIP_TRY(hipStreamWaitEvent(c->crit_side, c->crit_fork, 0));
    side_guard.st = c->crit_side;
    gmpc_launch_mlp_transpose_all(cd.head, c->crit_side);
    HIP_TRY(hipEventRecord(c->crit_tr, c->crit_side));
  }
  const gmpc_shape& sh = c->sh;
  const int n = c->nx, F = sh.lstm_features, T1 = sh.T + 1;
  // wide inputs (n + F > 256): x_t Wx for all steps is one MFMA GEMM up front and the LSTM kernels
  // run on the recurrent half only (cr: n = 0, Wcat = Wh); dx comes back through a second GEMM
  const bool widein = c->xT != nullptr;
  const int R = Bc * T1, G4w = 4 * F;
  CriticDesc cr = cd;
  auto gemm1 = [&](int M, int N, int K, const float* X, int ldx, const float* Y, int ldy, float* Cp,
                   int ldc) {
    gmpc_launch_bgemm_tn(bgemm_args(1, M, N, K, X, 0, ldx, Y, 0, ldy, Cp, 0, ldc, nullptr), s);
  };
  if (widein) {
    cr.n = 0;
    cr.Wcat = critic + (long)n * G4w;
    cr.WcatT = c->WhT;
    gmpc_launch_transpose(F, G4w, cr.Wcat, c->WhT, s);
  }
  const bool gen2 = !widein && c->lwp != nullptr && gmpc_lstm2_supported(cd);
  if (gen2) {
    ProfScope ps(c, PROF_LSTM_FWD, s);
    gmpc_launch_lstm_fwd2(Bc, cd, xseq, c->gates, c->cs, c->hp, c->hT, s);
  } else {
    ProfScope ps(c, PROF_LSTM_FWD, s);
    if (widein) {
      gmpc_launch_transpose(R, n, xseq, c->xT, s);                       // [R][n] -> [n][R]
      gemm1(R, G4w, n, c->xT, R, critic, G4w, c->xproj, G4w);             // xproj = x Wx
    }
    gmpc_launch_lstm_fwd(Bc, cr, xseq, c->gates, c->cs, c->hp, c->hT, widein ? c->xproj : nullptr, s);
  }
  if (tr_side) {
    HIP_TRY(hipStreamWaitEvent(s, c->crit_tr, 0));
    side_guard.st = nullptr;        // joined
  }
  {
    ProfScope ps(c, PROF_HEAD, s);
    gmpc_launch_head2(Bc, cd, loss_kind, c->hT, label, c->cscore, c->closs, c->hacts, c->hdels, c->plast, c->dhT,
                      c->hrows, s);
  }
  hipStream_t sw = s;
  bool forked = false;
  if (gen2 && want_wgrad && side_on) {
    HIP_TRY(hipEventRecord(c->crit_fork, s));
    HIP_TRY(hipStreamWaitEvent(c->crit_side, c->crit_fork, 0));
    sw = c->crit_side;
    forked = true;
    side_guard.st = c->crit_side;
  }
  float* gWx0 = grad_sum;
  if (gen2 && (dxseq || want_wgrad)) {
    // backward sweep with the LSTM weight gradients accumulated in registers (no dz in memory), then the
    // reduction of the per-workgroup partials straight into grad_sum
    ProfScope ps(c, PROF_LSTM_BWD, s);
    float* gWh0 = want_wgrad ? gWx0 + (long)n * 4 * F : nullptr;
    gmpc_launch_lstm_bwd2(Bc, cd, xseq, c->gates, c->cs, c->hp, c->dhT, want_wgrad ? c->lwp : nullptr, gWx0, gWh0,
                          want_wgrad ? gWh0 + (long)F * 4 * F : nullptr, dxseq, s);
  } else if (dxseq || want_wgrad) {
    ProfScope ps(c, PROF_LSTM_BWD, s);
    if (!widein) {
      gmpc_launch_lstm_bwd(Bc, cd, c->gates, c->cs, c->dhT, want_wgrad ? c->dz : nullptr, dxseq, s);
    } else {
      gmpc_launch_lstm_bwd(Bc, cr, c->gates, c->cs, c->dhT, c->dz, nullptr, s);
      if (dxseq) {
        gmpc_launch_transpose(R, G4w, c->dz, c->xproj, s);               // dz^T: [4F][R]
        gemm1(R, n, G4w, c->xproj, R, c->critT, n + F, dxseq, n);         // dx = dz Wx^T
      }
    }
  }
  if (want_wgrad) {
    ProfScope ps(c, PROF_WGRAD, sw);
    const int rows = Bc * T1, G4 = 4 * F;
    float* gWx = grad_sum;
    float* gWh = gWx + (long)n * G4;
    float* gb = gWh + (long)F * G4;
    // every problem with N % 256 == 0 goes into one batched launch (+ one reduction launch)
    WgProb pr[GMPC_WG_MAX];
    int np = 0;
    auto add = [&](int r, int M, int N, const float* A, int lda, const float* Bm, int ldb, float* Cw,
                   float* cs, int cs_rows) {
      WgProb q{};
      q.rows = r; q.M = M; q.N = N; q.lda = lda; q.ldb = ldb; q.cs_rows = cs_rows;
      q.A = A; q.B = Bm; q.C = Cw; q.colsum = cs;
      pr[np++] = q;
    };
    struct Single { int r, M, N; const float* A; int lda; const float* Bm; int ldb; float* Cw; float* cs; int csr; };
    Single single[GMPC_MAX_LAYERS + 2];
    int ns = 0;
    auto route = [&](int r, int M, int N, const float* A, int lda, const float* Bm, int ldb, float* Cw,
                     float* cs, int cs_rows) {
      if (N % 256 == 0 && r >= 64 && np < GMPC_WG_MAX) add(r, M, N, A, lda, Bm, ldb, Cw, cs, cs_rows);
      else single[ns++] = Single{r, M, N, A, lda, Bm, ldb, Cw, cs, cs_rows};
    };
    if (!gen2) {
      route(rows, n, G4, xseq, n, c->dz, G4, gWx, nullptr, 0);
      route(rows, F, G4, c->hp, F, c->dz, G4, gWh, gb, rows);
    }
    float* gh = gb + G4;
    for (int l = 0; l < sh.head_layers; ++l) {
      const int M = sh.head_dims[l], N = sh.head_dims[l + 1];
      if (l == sh.head_layers - 1 && np < GMPC_WG_MAX) {
        // the last layer has one output: its weight gradient and its bias gradient are the column sums of
        // k_head2's products [act * dscore | dscore] -- a problem without a GEMM part (M = 0)
        add(Bc, 0, M + 1, c->plast, GMPC_HEAD2_LD, c->plast, GMPC_HEAD2_LD, gh, gh, Bc);
      } else {
        route(Bc, M, N, c->hacts + c->hrows.aoff[l], c->hrows.stride, c->hdels + c->hrows.doff[l], c->hrows.stride, gh,
              gh + (long)M * N, Bc);
      }
      gh += (long)M * N + N;
    }
    if (np > 0 && !gmpc_launch_wgrad_batch(pr, np, c->wpart, c->wpart_floats, sw)) {
      for (int i = 0; i < np; ++i)
        single[ns++] = Single{pr[i].rows, pr[i].M, pr[i].N, pr[i].A, pr[i].lda, pr[i].B, pr[i].ldb, pr[i].C,
                              pr[i].colsum, pr[i].cs_rows};
    }
    // the rest one by one, after the batch (they reuse the partial-sum buffer: stream order)
    for (int i = 0; i < ns; ++i) {
      if (single[i].M == 0)
        gmpc_launch_colsum(single[i].csr, single[i].N, single[i].Bm, single[i].ldb, single[i].cs, c->wpart,
                           c->wpart_floats, sw);
      else
        gmpc_launch_wgrad(single[i].r, single[i].M, single[i].N, single[i].A, single[i].lda, single[i].Bm,
                          single[i].ldb, single[i].Cw, single[i].cs, single[i].csr, c->wpart, sw,
                          c->wpart_floats, true);
    }
  }
  if (loss_sum) gmpc_launch_sum(Bc, c->closs, loss_sum, 0, sw);
  if (forked) {
    HIP_TRY(hipEventRecord(c->crit_join, sw));
    HIP_TRY(hipStreamWaitEvent(s, c->crit_join, 0));
    side_guard.st = nullptr;        // joined
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int gmpc_critic_loss_grad(gmpc_ctx* c, int Bc, const float* xseq, const float* label,
                                     const float* critic, float* loss_sum, float* grad_sum,
                                     void* stream) {
  if (!c) return fail(GMPC_EINVAL, "ctx is null");
  if (Bc < 1 || Bc > 2 * c->maxB) return fail(GMPC_EINVAL, "Bc=%d outside [1, 2*max_batch]", Bc);
  if (!xseq || !label || !critic || !loss_sum || !grad_sum) return fail(GMPC_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(c->device));
  (void)hipGetLastError();   // clean slate (see check_call)
  hipStream_t s = static_cast<hipStream_t>(stream);
  TRY(critic_forward_backward(c, Bc, xseq, label, critic, 0, nullptr, true, grad_sum, s, loss_sum));
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int gmpc_critic_score_vjp(gmpc_ctx* c, int Bc, const float* xseq, const float* critic,
                                     float* score, float* dxseq, void* stream) {
  if (!c) return fail(GMPC_EINVAL, "ctx is null");
  if (Bc < 1 || Bc > 2 * c->maxB) return fail(GMPC_EINVAL, "Bc=%d outside [1, 2*max_batch]", Bc);
  if (!xseq || !critic || !score) return fail(GMPC_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(c->device));
  (void)hipGetLastError();   // clean slate (see check_call)
  hipStream_t s = static_cast<hipStream_t>(stream);
  TRY(critic_forward_backward(c, Bc, xseq, nullptr, critic, 2, dxseq, false, nullptr, s));
  HIP_TRY(hipMemcpyAsync(score, c->cscore, Bc * sizeof(float), hipMemcpyDeviceToDevice, s));
  return 0;
}

// The VJP of the score for a caller's output delta g_score = d loss / d score (k_head2 loss_kind 3): one forward
// sweep, one head pass, one backward pass on whichever route the shape takes.  Stateless: the critic's own workspace
// and the caller's outputs only.
extern "C" int gmpc_critic_vjp(gmpc_ctx* c, int Bc, const float* xseq, const float* critic, const float* g_score,
                               float* score, float* grad_xseq, float* grad_critic_sum, void* stream) {
  if (!c) return fail(GMPC_EINVAL, "ctx is null");
  if (c->sh.lstm_features <= 0) return fail(GMPC_EINVAL, "gmpc_critic_vjp: this ctx was created without a critic");
  if (Bc < 1 || Bc > 2 * c->maxB)
    return fail(GMPC_EINVAL, "gmpc_critic_vjp: Bc=%d outside [1, 2*max_batch=%d]", Bc, 2 * c->maxB);
  if (!xseq) return fail(GMPC_EINVAL, "gmpc_critic_vjp: xseq is null");
  if (!critic) return fail(GMPC_EINVAL, "gmpc_critic_vjp: critic is null");
  if (!g_score) return fail(GMPC_EINVAL, "gmpc_critic_vjp: g_score is null");
  if (!grad_xseq && !grad_critic_sum)
    return fail(GMPC_EINVAL, "gmpc_critic_vjp: grad_xseq and grad_critic_sum are both null");
  HIP_TRY(hipSetDevice(c->device));
  (void)hipGetLastError();   // clean slate (see check_call)
  hipStream_t s = static_cast<hipStream_t>(stream);
  TRY(critic_forward_backward(c, Bc, xseq, g_score, critic, 3, grad_xseq, grad_critic_sum != nullptr,
                              grad_critic_sum, s));
  if (score) HIP_TRY(hipMemcpyAsync(score, c->cscore, Bc * sizeof(float), hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipGetLastError());
  return 0;
}

// The second-order VJP of the scores (gmpc_critic_dir.hip): forward of (score, sdot = <d score / d x, v>), the tangent
// head's reverse for the caller's delta g_dir on sdot, the dual BPTT sweep, and the weight gradients as GEMMs over the
// rows the sweeps wrote.  Stateless as gmpc_critic_vjp; everything per call lives in the call workspace.
extern "C" int gmpc_critic_dir_vjp(gmpc_ctx* c, int Bc, const float* xseq, const float* critic, const float* v_xseq,
                                   const float* g_dir, float* score, float* sdot, float* grad_xseq,
                                   float* grad_critic_sum, void* stream) {
  if (!c) return fail(GMPC_EINVAL, "ctx is null");
  if (c->sh.lstm_features <= 0)
    return fail(GMPC_EINVAL, "gmpc_critic_dir_vjp: this ctx was created without a critic");
  if (Bc < 1 || Bc > 2 * c->maxB)
    return fail(GMPC_EINVAL, "gmpc_critic_dir_vjp: Bc=%d outside [1, 2*max_batch=%d]", Bc, 2 * c->maxB);
  if (!xseq) return fail(GMPC_EINVAL, "gmpc_critic_dir_vjp: xseq is null");
  if (!critic) return fail(GMPC_EINVAL, "gmpc_critic_dir_vjp: critic is null");
  if (!v_xseq) return fail(GMPC_EINVAL, "gmpc_critic_dir_vjp: v_xseq is null");
  if (!sdot) return fail(GMPC_EINVAL, "gmpc_critic_dir_vjp: sdot is null");
  if ((grad_xseq || grad_critic_sum) && !g_dir)
    return fail(GMPC_EINVAL, "gmpc_critic_dir_vjp: g_dir is null but a gradient output is not");
  const gmpc_shape& sh = c->sh;
  const int n = c->nx, F = sh.lstm_features, T1 = sh.T + 1, G4 = 4 * F, K = n + F;
  if (K > GMPC_THREADS)
    return fail(GMPC_EINVAL, "gmpc_critic_dir_vjp: unsupported shape: x_size + lstm_features = %d + %d > %d (the "
                "wide-input route)", n, F, GMPC_THREADS);
  HIP_TRY(hipSetDevice(c->device));
  (void)hipGetLastError();   // clean slate (see check_call)
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool want_w = grad_critic_sum != nullptr, want_grad = want_w || grad_xseq != nullptr;
  const size_t R = (size_t)Bc * T1;
  CriticDesc cd;
  cd.n = n; cd.F = F; cd.T1 = T1;
  if (!gmpc_dir_supported(cd))
    return fail(GMPC_EINVAL, "gmpc_critic_dir_vjp: unsupported shape: x_size = %d, lstm_features = %d", n, F);
  // the call's workspace first: an allocation failure leaves nothing in flight
  CallWork& w = c->cw;
  TRY(w.save.grow(c, gmpc_dir_save_floats(cd, Bc)));
  if (want_w) {
    TRY(w.acts.reserve(c, 2 * R, K, s));
    TRY(w.dels.reserve(c, 2 * R, G4, s));
  }
  if (want_grad) {
    TRY(w.acts2.reserve(c, Bc, c->hrows.stride, s));
    TRY(w.dels2.reserve(c, Bc, c->hrows.stride, s));
  }
  if (want_grad) {
    // the sweeps read [Wx; Wh]^T on every shape: bind_critic leaves it out where the register-weight kernels run
    TRY(bind_critic(c, critic, cd, s));
    if (c->lwp != nullptr && gmpc_lstm2_supported(cd)) gmpc_launch_transpose(K, G4, cd.Wcat, c->critT, s);
  } else {
    cd.Wcat = critic;
    cd.WcatT = nullptr;
    cd.b = critic + (long)K * G4;
    bind_mlp(cd.head, sh.head_layers, sh.head_dims, cd.b + G4, nullptr);
  }
  DirSaves sv;
  gmpc_dir_bind_saves(cd, Bc, w.save.p, &sv);
  sv.A = want_w ? w.acts.p : nullptr;
  {
    ProfScope ps(c, PROF_LSTM_FWD, s);
    gmpc_launch_dir_fwd(Bc, cd, xseq, v_xseq, sv, s);
  }
  {
    ProfScope ps(c, PROF_HEAD, s);
    gmpc_launch_dir_head(Bc, cd, sv, want_grad ? g_dir : nullptr, score, sdot, w.acts2.p, w.dels2.p, c->hrows, s);
  }
  if (want_grad) {
    ProfScope ps(c, PROF_LSTM_BWD, s);
    gmpc_launch_dir_bwd(Bc, cd, sv, want_w ? w.dels.p : nullptr, grad_xseq, s);
  }
  if (want_w) {
    ProfScope ps(c, PROF_WGRAD, s);
    // [gWx ; gWh] = A^T D over both halves of the rows, gb = the column sums of D's primal half
    float* gb = grad_critic_sum + (long)K * G4;
    const int rows = (int)(2 * R);
    WgProb q{};
    q.rows = rows; q.M = K; q.N = G4; q.lda = K; q.ldb = G4; q.cs_rows = (int)R;
    q.A = w.acts.p; q.B = w.dels.p; q.C = grad_critic_sum; q.colsum = gb;
    if (!(G4 % 256 == 0 && rows >= 64 && gmpc_launch_wgrad_batch(&q, 1, c->wpart, c->wpart_floats, s)))
      gmpc_launch_wgrad(rows, K, G4, w.acts.p, K, w.dels.p, G4, grad_critic_sum, gb, (int)R, c->wpart, s,
                        c->wpart_floats, true);
    // head: dW_l = sum_b ad_l^T d_l; the biases enter the tangent through the masks only: exact zeros
    float* gh = gb + G4;
    HIP_TRY(hipMemsetAsync(gh, 0, mlp_count(sh.head_layers, sh.head_dims) * sizeof(float), s));
    for (int l = 0; l < sh.head_layers; ++l) {
      const int M = sh.head_dims[l], N = sh.head_dims[l + 1];
      gmpc_launch_wgrad(Bc, M, N, w.acts2.p + c->hrows.aoff[l], c->hrows.stride, w.dels2.p + c->hrows.doff[l],
                        c->hrows.stride, gh, nullptr, 0, c->wpart, s, c->wpart_floats, true);
      gh += (long)M * N + N;
    }
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// upper-level loss only, at the solution held by the ctx (norm/cost_trainer.py:13-21 test loss)
int upper_loss(gmpc_ctx* c, int B, int loss_kind, const float* desired, const float* critic,
                      float* loss, bool want_lx, hipStream_t s) {
  const gmpc_shape& sh = c->sh;
  if (loss_kind == 0) {
    if (!desired) return fail(GMPC_EINVAL, "desired is null");
    gmpc_launch_l2loss(B, sh.T, sh.n, c->nx, c->Xs, desired, loss, c->lx, s);
  } else if (loss_kind == 1) {
    if (!critic) return fail(GMPC_EINVAL, "critic is null");
    if (c->dynl) {
      // the critic sees the x columns of xc (gan/js_policy.py:64-65); its input gradient goes back into
      // those columns, zero on the carry
      const long rows = (long)B * (sh.T + 1);
      gmpc_launch_cols_gather(rows, sh.n, c->nx, c->Xs, c->xg, s);
      TRY(critic_forward_backward(c, B, c->xg, nullptr, critic, 1, want_lx ? c->lxg : nullptr, false,
                                  nullptr, s));
      if (want_lx) gmpc_launch_cols_scatter(rows, sh.n, c->nx, c->lxg, c->lx, s);
    } else
    TRY(critic_forward_backward(c, B, c->Xs, nullptr, critic, 1, want_lx ? c->lx : nullptr, false,
                                nullptr, s));
    HIP_TRY(hipMemcpyAsync(loss, c->closs, B * sizeof(float), hipMemcpyDeviceToDevice, s));
  } else {
    return fail(GMPC_EINVAL, "loss_kind must be 0 (L2) or 1 (JS)");
  }
  return 0;
}

extern "C" int gmpc_upper_loss(gmpc_ctx* c, int B, int loss_kind, const float* desired,
                               const float* critic, float* loss, void* stream) {
  TRY(check_call(c, B));
  if (c->solB != B) return fail(GMPC_EINVAL, "gmpc_ilqr_solve with B=%d must precede this call", B);
  if (!loss) return fail(GMPC_EINVAL, "null argument");
  c->gradB = 0;   // the L2 loss rewrites the ctx's lx, which gmpc_bilevel_grad_inputs would read
  TRY(upper_loss(c, B, loss_kind, desired, critic, loss, false, static_cast<hipStream_t>(stream)));
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int gmpc_polyak(gmpc_ctx* c, long count, const float* prev, const float* cur, double factor,
                           float* out, void* stream) {
  if (!c || !prev || !cur || !out || count < 1) return fail(GMPC_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  (void)hipGetLastError();   // clean slate (see check_call)
  gmpc_launch_polyak(count, prev, cur, factor, out, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int gmpc_adam_clip_step(gmpc_ctx* c, long count, float* params, const float* grad,
                                   float* m, float* v, float grad_scale, int step, double lr,
                                   double max_norm, double b1, double b2, double eps, void* stream) {
  if (!c || !params || !grad || !m || !v) return fail(GMPC_EINVAL, "null argument");
  if (count < 1 || step < 1) return fail(GMPC_EINVAL, "count and step must be positive");
  HIP_TRY(hipSetDevice(c->device));
  (void)hipGetLastError();   // clean slate (see check_call)
  hipStream_t s = static_cast<hipStream_t>(stream);
  {
    ProfScope ps(c, PROF_ADAM, s);
    gmpc_launch_adam(count, params, grad, m, v, grad_scale, step, lr, max_norm, b1, b2, eps,
                     c->scratch, s);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// Batched TN GEMM (gmpc_bgemm.hip) used by the large-state Riccati path, exported for its unit test:
// C[b] = alpha * X[b]^T Y[b] + beta * C[b] with X[b] K x M, Y[b] K x N, C[b] M x N, all row-major
// and densely packed per batch element.  Y must be followed by >= 8 readable rows.
extern "C" int gmpc_bgemm_tn(gmpc_ctx* c, int batch, int M, int N, int K, const float* X, const float* Y,
                             float* C, float alpha, float beta, void* stream) {
  if (!c || !X || !Y || !C || batch < 1 || M < 1 || N < 1 || K < 1) return fail(GMPC_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  (void)hipGetLastError();   // clean slate (see check_call)
  gmpc_launch_bgemm_tn(bgemm_args(batch, M, N, K, X, (long)K * M, M, Y, (long)K * N, N, C, (long)M * N, N, nullptr,
                                  alpha, beta),
                       static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return 0;
}

// The same product with every field of BgemmArgs in the caller's hands (strides, leading dimensions, `active`, the
// further K-segments, the epilogue extras, `upper_only`): the entry point of tests/bgemm_cases.py.
static bool bgemm_desc_ok(const gmpc_bgemm_desc* d) {
  if (!d || !d->X || !d->Y || !d->C || d->batch < 1 || d->M < 1 || d->N < 1 || d->K < 1) return false;
  if (d->ldx < d->M || d->ldy < d->N || d->ldc < d->N || d->sx < 0 || d->sy < 0 || d->sc < 0) return false;
  if (d->K2 < 0 || (d->K2 > 0 && (!d->X2 || !d->Y2 || d->ldx2 < d->M || d->ldy2 < d->N))) return false;
  if (d->K3 < 0 || (d->K3 > 0 && (!d->X3 || !d->Y3 || d->ldx3 < d->M || d->ldy3 < d->N))) return false;
  if (d->E && (d->En < 0 || d->En > d->N || d->lde < d->En)) return false;
  if (d->upper_only && d->M != d->N) return false;
  return true;
}
static BgemmArgs bgemm_desc_args(const gmpc_bgemm_desc* d) {
  BgemmArgs g = bgemm_args(d->batch, d->M, d->N, d->K, d->X, d->sx, d->ldx, d->Y, d->sy, d->ldy, d->C, d->sc, d->ldc,
                           d->active, d->alpha, d->beta);
  g.X2 = d->X2; g.sx2 = d->sx2; g.ldx2 = d->ldx2; g.Y2 = d->Y2; g.sy2 = d->sy2; g.ldy2 = d->ldy2; g.K2 = d->K2;
  g.X3 = d->X3; g.sx3 = d->sx3; g.ldx3 = d->ldx3; g.Y3 = d->Y3; g.sy3 = d->sy3; g.ldy3 = d->ldy3; g.K3 = d->K3;
  g.upper_only = d->upper_only ? 1 : 0;
  g.E = d->E; g.se = d->se; g.lde = d->lde; g.En = d->En;
  g.rowmask = d->rowmask; g.srm = d->srm;
  return g;
}

extern "C" int gmpc_bgemm_tn_ex(gmpc_ctx* c, const gmpc_bgemm_desc* d, void* stream) {
  if (!c || !bgemm_desc_ok(d)) return fail(GMPC_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  (void)hipGetLastError();   // clean slate (see check_call)
  gmpc_launch_bgemm_tn(bgemm_desc_args(d), static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return 0;
}

// The kernel form gmpc_bgemm_tn_ex would launch for `d`; host only, the pointers are compared with NULL and never
// followed.
extern "C" int gmpc_bgemm_route(const gmpc_bgemm_desc* d, int* route4) {
  if (!bgemm_desc_ok(d) || !route4) return fail(GMPC_EINVAL, "bad argument");
  const BgemmRoute r = gmpc_bgemm_route_of(bgemm_desc_args(d));
  route4[0] = r.family; route4[1] = r.p[0]; route4[2] = r.p[1]; route4[3] = r.p[2];
  return 0;
}

// The weight-gradient GEMM (gmpc_wgrad.hip) with every argument of its launchers in the caller's hands, the partial-sum
// buffer included: the entry points of tests/wgrad_cases.py.
static bool wgrad_desc_ok(const gmpc_wgrad_desc* d, bool in_batch) {
  if (!d || !d->B || d->rows < 1 || d->N < 1 || d->ldb < d->N) return false;
  if (!in_batch && (!d->part || d->part_floats < 1)) return false;
  if (!in_batch && d->form == GMPC_WGRAD_COLSUM_ONLY) return d->colsum != nullptr;
  if (!in_batch && d->form != GMPC_WGRAD_AUTO) return false;
  if (d->colsum && (d->cs_rows < 1 || d->cs_rows > d->rows)) return false;
  if (in_batch && d->M == 0) return d->colsum != nullptr && d->C == d->colsum;
  return d->A && d->C && d->M >= 1 && d->lda >= d->M;
}
static WgradRoute wgrad_desc_route(const gmpc_wgrad_desc* d) {
  if (d->form == GMPC_WGRAD_COLSUM_ONLY) return gmpc_wgrad_route_of(d->rows, 0, d->N, true, d->rows, d->part_floats, false);
  return gmpc_wgrad_route_of(d->rows, d->M, d->N, d->colsum != nullptr, d->cs_rows, d->part_floats, d->mfma_ok != 0);
}
// the batch as the launcher takes it; false for a bad argument
static bool wgrad_desc_batch(const gmpc_wgrad_desc* probs, int np, std::vector<WgProb>& pr) {
  if (!probs || np < 1 || np > 64) return false;
  pr.assign(np, WgProb{});
  for (int i = 0; i < np; ++i) {
    const gmpc_wgrad_desc* d = probs + i;
    if (!wgrad_desc_ok(d, true)) return false;
    WgProb& q = pr[i];
    q.rows = d->rows; q.M = d->M; q.N = d->N; q.lda = d->lda; q.ldb = d->ldb; q.cs_rows = d->cs_rows;
    q.A = d->A; q.B = d->B; q.C = d->C; q.colsum = d->colsum;
  }
  return true;
}

extern "C" int gmpc_wgrad_ex(gmpc_ctx* c, const gmpc_wgrad_desc* d, void* stream) {
  if (!c || !wgrad_desc_ok(d, false)) return fail(GMPC_EINVAL, "bad argument");
  if (d->form == GMPC_WGRAD_COLSUM_ONLY && d->part_floats < d->N) return fail(GMPC_EINVAL, "part holds fewer than N floats");
  HIP_TRY(hipSetDevice(c->device));
  (void)hipGetLastError();   // clean slate (see check_call)
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (d->form == GMPC_WGRAD_COLSUM_ONLY)
    gmpc_launch_colsum(d->rows, d->N, d->B, d->ldb, d->colsum, d->part, d->part_floats, s);
  else
    gmpc_launch_wgrad(d->rows, d->M, d->N, d->A, d->lda, d->B, d->ldb, d->C, d->colsum, d->cs_rows, d->part, s,
                      d->part_floats, d->mfma_ok != 0);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int gmpc_wgrad_batch_ex(gmpc_ctx* c, const gmpc_wgrad_desc* probs, int np, float* part, long part_floats,
                                   void* stream, int* taken) {
  std::vector<WgProb> pr;
  if (!c || !part || part_floats < 1 || !taken || !wgrad_desc_batch(probs, np, pr)) return fail(GMPC_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  (void)hipGetLastError();   // clean slate (see check_call)
  *taken = gmpc_launch_wgrad_batch(pr.data(), np, part, part_floats, static_cast<hipStream_t>(stream)) ? 1 : 0;
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int gmpc_wgrad_route(const gmpc_wgrad_desc* d, int* route6) {
  if (!wgrad_desc_ok(d, false) || !route6) return fail(GMPC_EINVAL, "bad argument");
  const WgradRoute r = wgrad_desc_route(d);
  route6[0] = r.form; route6[1] = r.ntw; route6[2] = r.rpc; route6[3] = r.nchunks; route6[4] = r.crpc; route6[5] = r.cchunks;
  return 0;
}

extern "C" int gmpc_wgrad_batch_route(const gmpc_wgrad_desc* probs, int np, long part_floats, int* route2) {
  std::vector<WgProb> pr;
  if (part_floats < 1 || !route2 || !wgrad_desc_batch(probs, np, pr)) return fail(GMPC_EINVAL, "bad argument");
  route2[1] = gmpc_wgrad_batch_plan(pr.data(), np, part_floats);
  route2[0] = route2[1] != 0 ? 1 : 0;
  return 0;
}

// multi-GPU exchange -----------------------------------------------------------------------------
extern "C" int gmpc_comm_unique_id(char* id128) {
  if (!id128) return fail(GMPC_EINVAL, "null argument");
  return gmpc_comm_unique_id_impl(id128);
}

extern "C" int gmpc_comm_init(gmpc_ctx* c, int world_size, int rank, const char* id128) {
  if (!c || !id128) return fail(GMPC_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(c->device));
  return gmpc_comm_init_impl(&c->comm, world_size, rank, id128);
}

extern "C" int gmpc_allreduce_grads(gmpc_ctx* c, float* packed, long count, void* stream) {
  if (!c || !packed || count < 1) return fail(GMPC_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  return gmpc_comm_allreduce_impl(&c->comm, packed, count, static_cast<hipStream_t>(stream));
}

extern "C" int gmpc_comm_world(gmpc_ctx* c, int* world_size, int* rank) {
  if (!c || !world_size || !rank) return fail(GMPC_EINVAL, "null argument");
  *world_size = c->comm.world;
  *rank = c->comm.rank;
  return 0;
}
