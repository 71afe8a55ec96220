// The context behind the C ABI and what the files of its entry points share (gmpc_api*.hip; none of them has a kernel).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "gmpc_launch.h"

enum { PROF_ROLLOUT = 0, PROF_LINEARIZE, PROF_TERMINAL, PROF_RICCATI, PROF_LINESEARCH, PROF_LSTM_FWD,
       PROF_HEAD, PROF_LSTM_BWD, PROF_WGRAD, PROF_ADAM };

// error handling -------------------------------------------------------------------------------
static constexpr auto& fail = gmpc_fail;     // the entry points' name for the library's one error record
#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(GMPC_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                  __LINE__);                                                                \
  } while (0)
#define TRY(expr) do { int r_ = (expr); if (r_ != 0) return r_; } while (0)

#define GMPC_POLL_DEPTH 4   // iterations the host may enqueue ahead of the convergence flags it has seen

// A workspace buffer that an entry point sizes per call: grown to the largest size seen, never shrunk (the only
// allocations after gmpc_create)
struct GrowBuf {
  float* p = nullptr;
  size_t cap = 0;     // floats
  int grow(gmpc_ctx* c, size_t floats);
};
// Operand rows of the weight-gradient GEMM, [rows + GMPC_WGRAD_PAD][stride]: reserve() grows the buffer and zeroes the
// pad rows on `s` (the kernels that fill the buffer write the first `rows` rows only)
struct PadRows : GrowBuf {
  int reserve(gmpc_ctx* c, size_t rows, size_t stride, hipStream_t s);
};

// The workspace of one call of a gradient entry point (gmpc_expert_loss_grad, gmpc_bilevel_grad_dynamics,
// gmpc_rollout_vjp, gmpc_expert_vjp): each reserves what it needs at its top.  The contents are dead when the entry
// point returns, and calls on one context are stream-ordered (as the shared wpart / scratch already require), so every
// call may take all of it.  PadRows::reserve zeroes the pad rows on every call: that, not a first allocation, is what
// keeps them finite behind whatever an earlier call with other rows and another stride left there.
struct CallWork {
  PadRows acts, dels;     // the rows of the call's main network
  PadRows acts2, dels2;   // a second network's (gmpc_rollout_vjp: the cost MLP's)
  GrowBuf save, aux, aux2;
  GrowBuf part;           // the sampling solvers under an ensemble: the members' costs [P][B][ldc]
};

struct gmpc_ctx {
  gmpc_shape sh;
  GmpcComm comm;
  int nx = 0;            // x part of xc (= n unless the dynamics carry rides in xc)
  bool dynl = false;     // LSTM dynamics variant
  DynlDesc dl{};
  float *xg = nullptr, *lxg = nullptr;   // x columns of Xs / d loss / dx (critic-facing, dynl only)
  float* phi = nullptr;                  // dynl, small-state path: [B][T][n+m][n+m] curvature for the bilevel solve
  int maxB, device;
  int ncu = 0;           // compute units of `device` (the line search's plan sizes a pass over the chip with it)
  std::vector<void*> allocs;
  // bound parameters
  const float* mpc_w = nullptr;
  MlpDesc dyn{}, cost{};
  float *dynT = nullptr, *costT = nullptr, *linpad = nullptr;
  size_t linpad_floats = 0;
  LinPad lp{};
  bool params_set = false;
  // trajectory workspace
  uint32_t *masks, *maskc;
  float *Xc, *Uc, *AB, *QT, *qT;
  float *Xs, *Us, *goals, *Ks, *ks, *grads, *adjs;
  float *obj, *alpha, *obj_step, *U_step;
  int *iters, *cont;
  int* hcont = nullptr;                       // pinned ring of continuation flags (gmpc_ilqr_solve)
  float* fzcand = nullptr;                    // line-search candidates of gmpc_ilqr_solve_fused (shapes it covers)
  // gmpc_ilqr_solve_box's QP reports (same shapes): [B][2] cap hits / QP iterations of the solve, [B][T] QP
  // iterations and [B][T][m] clamped flags of the last backward pass
  float *box_count = nullptr, *box_iters = nullptr, *box_clamped = nullptr;
  // gmpc_ilqr_solve_box_held: [B][T] words, bit j = control j of the step is clamped at the held solution
  uint32_t* box_mask = nullptr;
  hipEvent_t poll_ev[GMPC_POLL_DEPTH] = {};
  int solB = 0;
  // the held solution is a box solve's: the bilevel tail differentiates through the active set in box_mask
  bool solBox = false;
  // batch size whose Bvec / H / dX (and Phi) a completed bilevel tail left for the held solution (0: none); every
  // change of the held solution clears it
  int gradB = 0;
  // bilevel workspace
  float *lx, *Bvec, *Hout, *dX, *gmpc, *cact, *cdel, *bl_loss;
  // acts / dels rows of the dynamics MLP (dynl: its tail), the cost MLP and the critic head
  MlpRows drows{}, crows{}, hrows{};
  // critic workspace
  float *critT, *gates, *cs, *hp, *hT, *dz, *hacts, *hdels, *dhT, *cscore, *closs;
  float* lwp = nullptr;        // weight-gradient partials of k_lstm_bwd2, one [85][256] block per 4 sequences
  // k_head2: last layer's act * dscore products and dscore, [Bc + GMPC_WGRAD_PAD][GMPC_HEAD2_LD]
  float* plast = nullptr;
  LsWork lsw{};
  // large-state (n > 64) backward pass
  bool big = false;
  BigWork bw{};
  float *WhT = nullptr, *xT = nullptr, *xproj = nullptr;   // wide-input critic (n + F > 256)
  // dynamics regression (allocated on first use)
  float *dfpred = nullptr, *dfacts = nullptr, *dfdels = nullptr, *dfloss = nullptr, *dfsave = nullptr;
  int dfstride = 0;
  float* efloss = nullptr;     // per-window losses of gmpc_expert_loss_grad
  CallWork cw;
  // gmpc_icem_solve: the device copy of the coloured sum's weights [T/2 + 1] and the noise_beta it was built for (the
  // upload is repeated only when noise_beta changes; icem_cw_host is what the asynchronous copy reads)
  float* icem_cw = nullptr;
  float icem_cw_beta = -1.f;
  std::vector<float> icem_cw_host;
  // gmpc_set_sampled_precision: the operand precision of the sampling solvers' sampled rollouts.  In bf16
  // mode dyn16 / cost16 are dyn / cost with W[l] pointing at the layers' packed bf16 images in w16 (allocated by the
  // first bf16-mode solve); gmpc_set_params marks them stale, the next bf16-mode solve packs them on its stream.
  int sampled_precision = GMPC_SAMPLED_FP32;
  void* w16 = nullptr;
  bool w16_stale = true;
  MlpDesc dyn16{}, cost16{};
  // gmpc_set_sampled_ensemble: ens_P > 0 members of the caller's [P][dyn count] vectors, under each of
  // which every launch over sampled rows rolls its rows out.  ens_dyn: member 0 bound like dyn (no transposes);
  // ens_dyn16: the same over the members' packed bf16 images in ens16 (P images of the dynamics, one behind the other;
  // grown and packed by the first bf16-mode solve behind every gmpc_set_sampled_ensemble).
  int ens_P = 0;
  MlpDesc ens_dyn{}, ens_dyn16{};
  GrowBuf ens16;
  bool ens16_stale = true;
  // gmpc_set_sampled_ensemble_mode: how the planes of a set ensemble are propagated and aggregated; read
  // by every launch over sampled rows, inert while ens_P == 0
  gmpc_ensemble_mode ens_mode{GMPC_ENS_MEAN, 0.f, GMPC_ENS_FIXED, 0};
  // gmpc_set_sampled_disagreement: the one-step disagreement penalty of the planes' costs; read by every
  // launch over sampled rows, inert while ens_P == 0, kept by gmpc_set_params and gmpc_set_sampled_ensemble
  int dis_kind = GMPC_DIS_OFF;
  float dis_penalty = 0.f;
  // shared scratch
  float *wpart, *scratch;
  long wpart_floats;
  // optional per-kernel timing with HIP events on the launch stream (gmpc_profile_*)
  bool prof = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_ev[GMPC_PROF_SLOTS];
  const char* lin_kernel = "";      // kernel the last Jacobian chain ran on (gmpc_profile_kernel_name)
  char lin_kernel_buf[96] = "";     // name of the chain instantiation this ctx launched last (copied at launch time)
  hipEvent_t lin_event = nullptr;   // caller's event, recorded after the Jacobian chain (gmpc_set_linearize_event)
  // the critic's head weight gradients run beside the BPTT sweep (critic_forward_backward): a context-owned side
  // stream forked after k_head2 and joined behind the sweep
  hipStream_t crit_side = nullptr;
  hipEvent_t crit_fork = nullptr, crit_join = nullptr, crit_tr = nullptr;
};

// RAII bracket: records a start/stop event pair around one kernel launch when profiling is on
struct ProfScope {
  gmpc_ctx* c; int slot; hipStream_t s; hipEvent_t e1 = nullptr;
  ProfScope(gmpc_ctx* c_, int slot_, hipStream_t s_) : c(c_), slot(slot_), s(s_) {
    if (!c->prof) return;
    hipEvent_t e0;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { e1 = nullptr; return; }
    (void)hipEventRecord(e0, s);
    c->prof_ev[slot].push_back({e0, e1});
  }
  ~ProfScope() { if (e1) (void)hipEventRecord(e1, s); }
};

template <typename Tp>
static int dalloc(gmpc_ctx* c, Tp** p, size_t count) {
  void* q = nullptr;
  if (count == 0) count = 1;
  hipError_t e = hipMalloc(&q, count * sizeof(Tp));
  if (e != hipSuccess)
    return fail(GMPC_ENOMEM, "hipMalloc(%zu bytes) failed: %s", count * sizeof(Tp),
                hipGetErrorString(e));
  c->allocs.push_back(q);
  *p = static_cast<Tp*>(q);
  return 0;
}

static long mlp_count(int L, const int* dims) {
  long c = 0;
  for (int l = 0; l < L; ++l) c += (long)dims[l] * dims[l + 1] + dims[l + 1];
  return c;
}

static void bind_mlp(MlpDesc& d, int L, const int* dims, const float* flat, float* flatT) {
  d.L = L;
  for (int l = 0; l <= L; ++l) d.dims[l] = dims[l];
  long off = 0;
  for (int l = 0; l < L; ++l) {
    d.W[l] = flat + off;
    d.WT[l] = flatT ? flatT + off : nullptr;
    off += (long)dims[l] * dims[l + 1];
    d.b[l] = flat + off;
    off += dims[l + 1];
  }
}

// The expert model of shape `es` in the flat vector `expert` = Wcat | bcat | head_x | head_u (expertT: the same layout
// for the transposed copies, or null), and the acts / dels row layout of its kernels.
static void bind_expert(ExpertNet& e, int nx, int m, const gmpc_expert_shape* es, const float* expert, float* expertT) {
  const int L = es->head_layers;
  e.n = nx; e.m = m; e.F = es->lstm_features; e.Y = es->head_dims_x[0];
  const long first = e.F > 0 ? (long)(nx + e.F) * 4 * e.F : (long)nx * e.Y, nb = e.F > 0 ? 4 * e.F : e.Y;
  const long hx_off = first + nb, hu_off = hx_off + mlp_count(L, es->head_dims_x);
  e.Wcat = expert;
  e.bcat = expert + first;
  e.WcatT = expertT;
  bind_mlp(e.hx, L, es->head_dims_x, expert + hx_off, expertT ? expertT + hx_off : nullptr);
  bind_mlp(e.hu, L, es->head_dims_u, expert + hu_off, expertT ? expertT + hu_off : nullptr);
  // acts row: [x_in | h_prev | y | head_x inputs a_1.. | head_u inputs a_1..]; dels row: [dz or d y_pre | head_x output
  // deltas | head_u output deltas]
  int off = nx + e.F + e.Y;
  e.ax[0] = e.au[0] = nx + e.F;
  for (int l = 1; l < L; ++l) { e.ax[l] = off; off += e.hx.dims[l]; }
  for (int l = 1; l < L; ++l) { e.au[l] = off; off += e.hu.dims[l]; }
  const int in_w = off;
  off = (int)nb;
  for (int l = 0; l < L; ++l) { e.dx[l] = off; off += e.hx.dims[l + 1]; }
  for (int l = 0; l < L; ++l) { e.du[l] = off; off += e.hu.dims[l + 1]; }
  e.stride = in_w > off ? in_w : off;
  e.hw = 1;
  for (int l = 0; l <= L; ++l) {
    e.hw = e.hx.dims[l] > e.hw ? e.hx.dims[l] : e.hw;
    e.hw = e.hu.dims[l] > e.hw ? e.hu.dims[l] : e.hw;
  }
}

// gmpc_api.hip: argument and state checks every entry point starts with
int check_call(gmpc_ctx* c, int B, bool need_params = true);
// gmpc_api.hip: c->lin_kernel after a launch of the chain `family` (LIN_* of gmpc_launch.h)
void set_lin_kernel(gmpc_ctx* c, int family);
// gmpc_api_sampled.hip: the sampling solvers' shared checks (`who`: the message's prefix) and the noise stream of
// iteration `it` under `seed` (beta: the smoothing along time)
int gmpc_sampled_coverage(const gmpc_ctx* c, const char* who);
// in bf16 mode: the packed weight images brought up to date on `s` (allocated on first use); nothing in fp32 mode
int gmpc_sampled_prepare(gmpc_ctx* c, hipStream_t s);
int gmpc_mppi_check_opts(const gmpc_mppi_opts* o);
CemRng gmpc_sampled_rng(uint64_t seed, int it, float beta);
// gmpc_api_critic.hip: the upper-level loss at the solution held by the ctx (and, with want_lx, its gradient in c->lx)
int upper_loss(gmpc_ctx* c, int B, int loss_kind, const float* desired, const float* critic, float* loss, bool want_lx,
               hipStream_t s);
