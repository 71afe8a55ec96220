// C-ABI entry points of the sampling solvers: the cross-entropy method, MPPI and the
// sample-efficient cross-entropy method on one sampled rollout (gmpc_launch_sampled_rollout), its precision, its
// dynamics ensemble, the ensemble's mode and its disagreement penalty.  What the three solves share is written once,
// ahead of them.
#include "gmpc_ctx.h"

// The shapes the sampled rollout covers, for the sampling solvers (`who`: the message's prefix)
int gmpc_sampled_coverage(const gmpc_ctx* c, const char* who) {
  const gmpc_shape& sh = c->sh;
  const int W = GMPC_SAMPLED_MAX_WIDTH;
  if (c->dynl) return fail(GMPC_EINVAL, "%s: MLP dynamics only (dyn_lstm_features = %d)", who, sh.dyn_lstm_features);
  for (int l = 0; l <= sh.dyn_layers; ++l)
    if (sh.dyn_dims[l] > W) return fail(GMPC_EINVAL, "%s: dynamics width %d above %d", who, sh.dyn_dims[l], W);
  for (int l = 0; l <= sh.cost_layers; ++l)
    if (sh.cost_dims[l] > W) return fail(GMPC_EINVAL, "%s: cost width %d above %d", who, sh.cost_dims[l], W);
  if (sh.n + sh.m > W) return fail(GMPC_EINVAL, "%s: n + m = %d above %d", who, sh.n + sh.m, W);
  return 0;
}

extern "C" int gmpc_set_sampled_precision(gmpc_ctx* c, int precision) {
  if (!c) return fail(GMPC_EINVAL, "ctx is null");
  if (precision != GMPC_SAMPLED_FP32 && precision != GMPC_SAMPLED_BF16)
    return fail(GMPC_EINVAL, "sampled precision: %d is neither GMPC_SAMPLED_FP32 (0) nor GMPC_SAMPLED_BF16 (1)",
                precision);
  c->sampled_precision = precision;
  return 0;
}

// The dynamics ensemble of the sampled rollouts: the pointer is kept, not owned, and nothing is launched
extern "C" int gmpc_set_sampled_ensemble(gmpc_ctx* c, int P, const float* dyn_members) {
  if (!c) return fail(GMPC_EINVAL, "ensemble: ctx is null");
  if (P < 0 || P > GMPC_MAX_ENSEMBLE)
    return fail(GMPC_EINVAL, "ensemble: P = %d outside [0, %d]", P, GMPC_MAX_ENSEMBLE);
  if (P == 0) {
    c->ens_P = 0;
    return 0;
  }
  if (!dyn_members) return fail(GMPC_EINVAL, "ensemble: dyn_members is null with P = %d", P);
  TRY(gmpc_sampled_coverage(c, "ensemble"));
  bind_mlp(c->ens_dyn, c->sh.dyn_layers, c->sh.dyn_dims, dyn_members, nullptr);
  c->ens_P = P;
  c->ens16_stale = true;   // the members changed: their bf16 images are packed again by the next bf16-mode solve
  return 0;
}

// How a set ensemble is propagated and aggregated: checked whole, then stored; nothing is launched
extern "C" int gmpc_set_sampled_ensemble_mode(gmpc_ctx* c, const gmpc_ensemble_mode* mode) {
  if (!c) return fail(GMPC_EINVAL, "ensemble mode: ctx is null");
  if (!mode) return fail(GMPC_EINVAL, "ensemble mode: mode is null");
  const gmpc_ensemble_mode& m = *mode;
  if (m.aggregate < GMPC_ENS_MEAN || m.aggregate > GMPC_ENS_MAX)
    return fail(GMPC_EINVAL, "ensemble mode: aggregate = %d outside [0, 2]", m.aggregate);
  if (m.propagation != GMPC_ENS_FIXED && m.propagation != GMPC_ENS_TS1)
    return fail(GMPC_EINVAL, "ensemble mode: propagation = %d outside [0, 1]", m.propagation);
  if (!std::isfinite(m.risk)) return fail(GMPC_EINVAL, "ensemble mode: risk = %g is not finite", (double)m.risk);
  if (m.risk != 0.f && m.aggregate != GMPC_ENS_MEAN_STD)
    return fail(GMPC_EINVAL, "ensemble mode: risk = %g goes with GMPC_ENS_MEAN_STD only (aggregate = %d)",
                (double)m.risk, m.aggregate);
  if (m.propagation == GMPC_ENS_FIXED && m.particles != 0)
    return fail(GMPC_EINVAL, "ensemble mode: particles = %d goes with GMPC_ENS_TS1 only", m.particles);
  if (m.propagation == GMPC_ENS_TS1 && (m.particles < 1 || m.particles > GMPC_MAX_ENSEMBLE))
    return fail(GMPC_EINVAL, "ensemble mode: particles = %d outside [1, %d]", m.particles, GMPC_MAX_ENSEMBLE);
  c->ens_mode = m;
  return 0;
}

// The one-step disagreement penalty of a set ensemble's planes: checked whole, then stored; nothing is
// launched
extern "C" int gmpc_set_sampled_disagreement(gmpc_ctx* c, int kind, float penalty) {
  if (!c) return fail(GMPC_EINVAL, "disagreement: ctx is null");
  if (kind != GMPC_DIS_OFF && kind != GMPC_DIS_ONESTEP)
    return fail(GMPC_EINVAL, "disagreement: kind = %d outside [0, 1]", kind);
  if (!std::isfinite(penalty)) return fail(GMPC_EINVAL, "disagreement: penalty = %g is not finite", (double)penalty);
  if (kind == GMPC_DIS_OFF && penalty != 0.f)
    return fail(GMPC_EINVAL, "disagreement: penalty = %g goes with GMPC_DIS_ONESTEP only", (double)penalty);
  TRY(gmpc_sampled_coverage(c, "disagreement"));
  c->dis_kind = kind;
  c->dis_penalty = penalty;
  return 0;
}

// What a solve refuses of the context's ensemble settings before its first launch: the disagreement measures a member
// against the nominal model along one rollout, which the per-step member draws of TS1 do not have
static int check_disagreement(const gmpc_ctx* c) {
  if (c->dis_kind != GMPC_DIS_OFF && c->ens_P > 0 && c->ens_mode.propagation == GMPC_ENS_TS1)
    return fail(GMPC_EINVAL, "disagreement: not with TS1 propagation");
  return 0;
}

// bf16 mode: the packed bf16 images of both MLPs, allocated by the first call and packed again behind
// every gmpc_set_params (one launch on `s`, ahead of the solve's own); called behind gmpc_sampled_coverage
int gmpc_sampled_prepare(gmpc_ctx* c, hipStream_t s) {
  if (c->sampled_precision != GMPC_SAMPLED_BF16) return 0;
  const gmpc_shape& sh = c->sh;
  if (!c->w16) {
    __bf16* p = nullptr;
    TRY(dalloc(c, &p, gmpc_bf16_image_elems(sh.dyn_layers, sh.dyn_dims) +
                          gmpc_bf16_image_elems(sh.cost_layers, sh.cost_dims)));
    c->w16 = p;
    c->w16_stale = true;
  }
  if (c->w16_stale) {
    gmpc_bind_bf16_images(c->dyn16, c->dyn, c->w16);
    gmpc_bind_bf16_images(c->cost16, c->cost,
                          static_cast<__bf16*>(c->w16) + gmpc_bf16_image_elems(sh.dyn_layers, sh.dyn_dims));
    gmpc_launch_pack_bf16(c->dyn, c->dyn16, c->cost, c->cost16, s);
    HIP_TRY(hipGetLastError());
    c->w16_stale = false;
  }
  if (c->ens_P > 0 && (c->ens16_stale || !c->ens16.p)) {
    // the members' images, one behind the other (each a multiple of 8 elements): k_pack_bf16 once per member, the
    // dynamics layers only (the cost MLP's image is the shared one above)
    const size_t elems = gmpc_bf16_image_elems(sh.dyn_layers, sh.dyn_dims);
    const long count = mlp_count(sh.dyn_layers, sh.dyn_dims);
    TRY(c->ens16.grow(c, (size_t)c->ens_P * elems / 2));
    gmpc_bind_bf16_images(c->ens_dyn16, c->ens_dyn, c->ens16.p);
    MlpDesc none{};
    for (int p = 0; p < c->ens_P; ++p) {
      MlpDesc src = c->ens_dyn, img = c->ens_dyn16;
      for (int l = 0; l < src.L; ++l) {
        src.W[l] += (size_t)p * count;
        img.W[l] += (size_t)p * (elems / 2);
      }
      gmpc_launch_pack_bf16(src, img, none, none, s);
    }
    HIP_TRY(hipGetLastError());
    c->ens16_stale = false;
  }
  return 0;
}

// What the launches over sampled rows need under an ensemble: the members' strides in the context's precision, the
// context's mode and the cost planes [Q][B][ldc] in the call workspace
static int ensemble_args(gmpc_ctx* c, int B, int ldc, CemEnsemble& e) {
  const gmpc_shape& sh = c->sh;
  const bool bf16 = c->sampled_precision == GMPC_SAMPLED_BF16;
  e.P = c->ens_P;
  e.bstride = (size_t)mlp_count(sh.dyn_layers, sh.dyn_dims);
  e.wstride = bf16 ? gmpc_bf16_image_elems(sh.dyn_layers, sh.dyn_dims) / 2 : e.bstride;
  e.ts1 = c->ens_mode.propagation == GMPC_ENS_TS1;
  e.Q = e.ts1 ? c->ens_mode.particles : c->ens_P;
  e.aggregate = c->ens_mode.aggregate;
  e.risk = c->ens_mode.risk;
  e.invQ = 1.0f / (float)e.Q;
  e.disagree = c->dis_kind == GMPC_DIS_ONESTEP;
  e.penalty = c->dis_penalty;
  memset(&e.nom, 0, sizeof(e.nom));
  if (e.disagree) {
    const MlpDesc& nd = bf16 ? c->dyn16 : c->dyn;
    for (int l = 0; l < nd.L; ++l) {
      e.nom.W[l] = nd.W[l];
      e.nom.b[l] = nd.b[l];
    }
  }
  TRY(c->cw.part.grow(c, (size_t)e.Q * B * ldc));
  e.part = c->cw.part.p;
  return 0;
}

// ---- what the three solves share ---------------------------------------------------------------------------------
static CemRollArgs& roll_of(CemRollArgs& r) { return r; }
static CemRollArgs& roll_of(IcemRollArgs& r) { return r.c; }
static int ldc_of(const CemRollArgs& r) { return r.N; }
static int ldc_of(const IcemRollArgs& r) { return r.ldc; }

// One launch over sampled rows (CEM's or iCEM's pool) in the context's precision (bf16 mode: the same arguments over
// the packed images).  With an ensemble set: the rows under every member or particle, then the
// reduce of the planes' costs into r's.
template <typename Args>
static int launch_sampled_rows(gmpc_ctx* c, const Args& r, hipStream_t s) {
  const bool bf16 = c->sampled_precision == GMPC_SAMPLED_BF16, ens = c->ens_P > 0;
  Args h = r;
  CemRollArgs& hc = roll_of(h);
  CemEnsemble e;
  if (ens && ensemble_args(c, hc.B, ldc_of(h), e)) return 1;
  if (ens) hc.dyn = bf16 ? c->ens_dyn16 : c->ens_dyn;
  else if (bf16) hc.dyn = c->dyn16;
  if (bf16) hc.cost = c->cost16;
  return gmpc_launch_sampled_rollout(h, bf16, ens ? &e : nullptr, s);
}

// The option ranges that the solvers share, in the order each of them checks its options
static int check_counts(const char* who, int num_samples, const int* num_elites) {
  if (num_samples < 1 || num_samples > GMPC_CEM_MAX_N)
    return fail(GMPC_EINVAL, "%s: num_samples = %d outside [1, %d]", who, num_samples, GMPC_CEM_MAX_N);
  if (num_elites && (*num_elites < 1 || *num_elites > num_samples))
    return fail(GMPC_EINVAL, "%s: num_elites = %d outside [1, num_samples = %d]", who, *num_elites, num_samples);
  return 0;
}
static int check_max_iter(const char* who, int max_iter) {
  if (max_iter < 0) return fail(GMPC_EINVAL, "%s: max_iter = %d is negative", who, max_iter);
  return 0;
}
static int check_smoothing(const char* who, const float* sampling, float evolution) {
  if (sampling && !(*sampling >= 0.f && *sampling < 1.f))
    return fail(GMPC_EINVAL, "%s: sampling_smoothing = %g outside [0, 1)", who, (double)*sampling);
  if (!(evolution >= 0.f && evolution <= 1.f))
    return fail(GMPC_EINVAL, "%s: evolution_smoothing = %g outside [0, 1]", who, (double)evolution);
  return 0;
}

// The noise stream of iteration `it` under `seed` (beta: the smoothing along time)
CemRng gmpc_sampled_rng(uint64_t seed, int it, float beta) {
  CemRng g;
  g.key0 = (uint32_t)(seed & 0xFFFFFFFFull); g.key1 = (uint32_t)(seed >> 32);
  g.it = (uint32_t)it;
  g.beta = beta;
  g.cbeta = sqrtf(1.f - beta * beta);
  return g;
}

// The head of a solve, behind the solver's checks of its own options: the bf16 images brought up to date and, where
// the caller gave no cost buffer, one of `cost_floats` floats from the call workspace -- both only with an iteration
static int sampled_begin(gmpc_ctx* c, int max_iter, size_t cost_floats, float** cost_buf, hipStream_t s) {
  if (max_iter <= 0) return 0;
  TRY(gmpc_sampled_prepare(c, s));
  if (!*cost_buf) {
    TRY(c->cw.aux.grow(c, cost_floats));
    *cost_buf = c->cw.aux.p;
  }
  return 0;
}

// The rollout arguments every solver fills from the context and its caller's arrays (costs, samples and the noise
// stream are per iteration)
static CemRollArgs sampled_roll_args(const gmpc_ctx* c, int B, int N, const float* x0, const float* goal,
                                     const float* mean, const float* sd, const float* lo, const float* hi) {
  const gmpc_shape& sh = c->sh;
  CemRollArgs r;
  memset(&r, 0, sizeof(r));
  r.B = B; r.N = N; r.T = sh.T; r.n = sh.n; r.m = sh.m;
  r.dyn = c->dyn; r.cost = c->cost; r.mpc_w = c->mpc_w;
  r.x0 = x0; r.goal = goal; r.mean = mean; r.sd = sd; r.lo = lo; r.hi = hi;
  return r;
}

// The tail of a solve: the returned sequence's own rollout -- one row per problem, no noise, no clamp (the mean_row
// form: fp32, the nominal model) -- where the caller asked for X or obj.  r: the solve's rollout arguments as its last
// iteration left them; seq [B][T][m].
static int sampled_finish(gmpc_ctx* c, const char* who, CemRollArgs r, const float* seq, float* X, float* obj,
                          hipStream_t s) {
  if (X || obj) {
    if (!obj) {
      TRY(c->cw.aux2.grow(c, (size_t)r.B));
      obj = c->cw.aux2.p;
    }
    r.N = 1; r.mean_row = 1; r.samples = nullptr; r.costs = obj; r.X = X; r.mean = seq;
    if (gmpc_launch_sampled_rollout(r, false, nullptr, s)) return fail(GMPC_EINVAL, "%s: shape not covered", who);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

// ---- the solves --------------------------------------------------------------------------------------------------
// The cross-entropy method: 2 max_iter + 1 launches on the caller's stream (3 max_iter + 1 under an
// ensemble, DESIGN §24: the reduce of the members' costs), nothing waited for.
// Stateless: it writes the caller's arrays and the call workspace only, so a held solution survives it.
extern "C" int gmpc_cem_solve(gmpc_ctx* c, int B, const float* x0, const float* goal, const float* u_lo,
                              const float* u_hi, const gmpc_cem_opts* o, float* mean_io, float* std_io, float* X,
                              float* obj, float* costs, int* elites, float* samples, void* stream) {
  TRY(check_call(c, B));
  TRY(gmpc_sampled_coverage(c, "cem"));
  TRY(check_disagreement(c));
  if (!o) return fail(GMPC_EINVAL, "cem: opts is null");
  if (!x0 || !goal || !mean_io || !std_io) return fail(GMPC_EINVAL, "cem: x0, goal, mean_io and std_io must not be null");
  TRY(check_counts("cem", o->num_samples, &o->num_elites));
  TRY(check_max_iter("cem", o->max_iter));
  TRY(check_smoothing("cem", &o->sampling_smoothing, o->evolution_smoothing));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int N = o->num_samples;
  float* cost_buf = costs;
  TRY(sampled_begin(c, o->max_iter, (size_t)B * N, &cost_buf, s));
  CemRollArgs r = sampled_roll_args(c, B, N, x0, goal, mean_io, std_io, u_lo, u_hi);
  r.rng = gmpc_sampled_rng(o->seed, 0, o->sampling_smoothing);
  r.costs = cost_buf;
  CemUpdArgs u;
  memset(&u, 0, sizeof(u));
  u.B = B; u.N = N; u.E = o->num_elites; u.T = r.T; u.m = r.m;
  u.costs = cost_buf; u.lo = u_lo; u.hi = u_hi; u.mean = mean_io; u.sd = std_io;
  u.gamma = o->evolution_smoothing;
  for (int i = 0; i < o->max_iter; ++i) {
    const bool last = i == o->max_iter - 1;
    r.rng.it = (uint32_t)(o->iter_offset + i);
    r.samples = last ? samples : nullptr;
    u.rng = r.rng;
    u.elites = last ? elites : nullptr;
    if (launch_sampled_rows(c, r, s) || gmpc_launch_cem_update(u, s)) return fail(GMPC_EINVAL, "cem: shape not covered");
  }
  return sampled_finish(c, "cem", r, mean_io, X, obj, s);
}

// What gmpc_mppi_solve and gmpc_mppi_vjp refuse in their options
int gmpc_mppi_check_opts(const gmpc_mppi_opts* o) {
  if (!o) return fail(GMPC_EINVAL, "mppi: opts is null");
  TRY(check_counts("mppi", o->num_samples, nullptr));
  TRY(check_max_iter("mppi", o->max_iter));
  TRY(check_smoothing("mppi", &o->sampling_smoothing, o->evolution_smoothing));
  if (!(o->temperature > 0.f) || !(o->temperature < INFINITY))
    return fail(GMPC_EINVAL, "mppi: temperature = %g is not positive and finite", (double)o->temperature);
  return 0;
}

// Model-predictive path integral control: CEM's samples and costs (the same rollout, unchanged), the elite
// cut replaced by softmax weights.  2 max_iter + 1 launches on the caller's stream, nothing waited for; stateless as
// gmpc_cem_solve is.
extern "C" int gmpc_mppi_solve(gmpc_ctx* c, int B, const float* x0, const float* goal, const float* u_lo,
                               const float* u_hi, const gmpc_mppi_opts* o, float* mean_io, const float* std, float* X,
                               float* obj, float* costs, float* weights, float* samples, float* means_trace,
                               float* costs_trace, void* stream) {
  TRY(check_call(c, B));
  TRY(gmpc_sampled_coverage(c, "mppi"));
  TRY(check_disagreement(c));
  TRY(gmpc_mppi_check_opts(o));
  if (!x0 || !goal || !mean_io || !std) return fail(GMPC_EINVAL, "mppi: x0, goal, mean_io and std must not be null");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int N = o->num_samples;
  const size_t BN = (size_t)B * N, BTm = (size_t)B * c->sh.T * c->sh.m;
  // with a trace the iteration's costs are written where they stay; `costs` gets the last iteration's copy
  float* cost_buf = costs_trace ? costs_trace : costs;
  TRY(sampled_begin(c, o->max_iter, BN, &cost_buf, s));
  CemRollArgs r = sampled_roll_args(c, B, N, x0, goal, mean_io, std, u_lo, u_hi);
  MppiUpdArgs u;
  memset(&u, 0, sizeof(u));
  u.B = B; u.N = N; u.T = r.T; u.m = r.m;
  u.lo = u_lo; u.hi = u_hi; u.mean = mean_io; u.sd = std;
  u.gamma = o->evolution_smoothing; u.lam = o->temperature;
  for (int i = 0; i < o->max_iter; ++i) {
    const bool last = i == o->max_iter - 1;
    r.rng = gmpc_sampled_rng(o->seed, o->iter_offset + i, o->sampling_smoothing);
    r.samples = last ? samples : nullptr;
    r.costs = costs_trace ? costs_trace + (size_t)i * BN : cost_buf;
    u.rng = r.rng;
    u.costs = r.costs;
    u.costs_copy = last && costs_trace ? costs : nullptr;
    u.weights = last ? weights : nullptr;
    u.mean_trace = means_trace ? means_trace + (size_t)i * BTm : nullptr;
    if (launch_sampled_rows(c, r, s) || gmpc_launch_mppi_update(u, s))
      return fail(GMPC_EINVAL, "mppi: shape not covered");
  }
  return sampled_finish(c, "mppi", r, mean_io, X, obj, s);
}

// What gmpc_icem_solve and gmpc_icem_plan_host refuse in their options
static int icem_check_opts(const gmpc_icem_opts* o) {
  if (!o) return fail(GMPC_EINVAL, "icem: opts is null");
  TRY(check_counts("icem", o->num_samples, &o->num_elites));
  if (o->num_keep < 0 || o->num_keep > o->num_elites)
    return fail(GMPC_EINVAL, "icem: num_keep = %d outside [0, num_elites = %d]", o->num_keep, o->num_elites);
  if (o->carry_in < 0 || o->carry_in > o->num_keep)
    return fail(GMPC_EINVAL, "icem: carry_in = %d outside [0, num_keep = %d]", o->carry_in, o->num_keep);
  if (o->num_samples + o->num_keep + 1 > GMPC_CEM_MAX_N)
    return fail(GMPC_EINVAL, "icem: num_samples + num_keep + 1 = %d above %d", o->num_samples + o->num_keep + 1,
                GMPC_CEM_MAX_N);
  TRY(check_max_iter("icem", o->max_iter));
  if (o->iter_offset < 0) return fail(GMPC_EINVAL, "icem: iter_offset = %d is negative", o->iter_offset);
  if (!(o->decay >= 1.f) || !(o->decay < INFINITY))
    return fail(GMPC_EINVAL, "icem: decay = %g is not finite and >= 1", (double)o->decay);
  if (!(o->noise_beta >= 0.f) || !(o->noise_beta < INFINITY))
    return fail(GMPC_EINVAL, "icem: noise_beta = %g is not finite and >= 0", (double)o->noise_beta);
  return check_smoothing("icem", nullptr, o->evolution_smoothing);
}

// The one place the sample counts and the coloured sum's weights are computed (host only; IEEE double arithmetic, so a
// NumPy restatement agrees: N_it exactly, cw to the rounding of libm's pow)
extern "C" int gmpc_icem_plan_host(const gmpc_icem_opts* o, int T, int* N_it, float* cw) {
  TRY(icem_check_opts(o));
  if (T < 1) return fail(GMPC_EINVAL, "icem: T = %d is not positive", T);
  if (N_it) {
    const double decay = (double)o->decay;
    const int floor_n = std::min(o->num_samples, 2 * o->num_elites);
    double nk = (double)o->num_samples;
    for (int it = 0; it < o->iter_offset && nk >= 1.0; ++it) nk = nk / decay;     // (below 1 the floor stays 0)
    for (int i = 0; i < o->max_iter; ++i) {
      N_it[i] = std::max((int)std::floor(nk), floor_n);
      nk = nk / decay;
    }
  }
  if (cw) {
    const int Kf = T / 2;
    std::vector<double> w(Kf + 1, 1.0);
    for (int k = 1; k <= Kf; ++k) w[k] = std::pow((double)k / (double)T, -(double)o->noise_beta / 2.0);
    if (Kf >= 1) w[0] = w[1];
    double s2 = w[0] * w[0];
    for (int k = 1; 2 * k < T; ++k) s2 += 2.0 * w[k] * w[k];
    if (T % 2 == 0) s2 += w[Kf] * w[Kf];
    const double s = std::sqrt(s2);
    cw[0] = (float)(w[0] / s);
    for (int k = 1; 2 * k < T; ++k) cw[k] = (float)(std::sqrt(2.0) * w[k] / s);
    if (T % 2 == 0) cw[Kf] = (float)(w[Kf] / s);
  }
  return 0;
}

// The sample-efficient cross-entropy method: 2 max_iter + 1 launches on the caller's stream, nothing
// waited for.  Stateless as gmpc_cem_solve is: the caller's arrays and the call workspace only.
extern "C" int gmpc_icem_solve(gmpc_ctx* c, int B, const float* x0, const float* goal, const float* u_lo,
                               const float* u_hi, const gmpc_icem_opts* o, float* mean_io, float* std_io,
                               float* keep_io, float* best_U_io, float* best_cost_io, float* U_out, float* X, float* obj,
                               float* costs, int* elites, float* samples, void* stream) {
  TRY(check_call(c, B));
  const gmpc_shape& sh = c->sh;
  TRY(gmpc_sampled_coverage(c, "icem"));
  TRY(check_disagreement(c));
  TRY(icem_check_opts(o));
  if (!x0 || !goal || !mean_io || !std_io)
    return fail(GMPC_EINVAL, "icem: x0, goal, mean_io and std_io must not be null");
  if (o->num_keep > 0 && !keep_io) return fail(GMPC_EINVAL, "icem: keep_io must not be null with num_keep = %d", o->num_keep);
  if ((best_U_io != nullptr) != (best_cost_io != nullptr))
    return fail(GMPC_EINVAL, "icem: best_U_io and best_cost_io go together");
  if (o->return_best && (!best_U_io || !U_out))
    return fail(GMPC_EINVAL, "icem: best_U_io, best_cost_io and U_out must not be null with return_best");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int N = o->num_samples, nk = o->num_keep, K = o->max_iter, T = sh.T, m = sh.m;
  const int ldc = N + nk + 1;
  const size_t BTm = (size_t)B * T * m, keep_floats = (size_t)B * nk * T * m;
  float* cost_buf = costs;
  TRY(sampled_begin(c, K, (size_t)B * ldc, &cost_buf, s));
  std::vector<int> Nit(K > 0 ? K : 1);
  std::vector<float> cwh(T / 2 + 1);
  TRY(gmpc_icem_plan_host(o, T, Nit.data(), cwh.data()));
  const bool white = o->noise_beta == 0.f || T < 2;
  if (!white && K > 0 && (!c->icem_cw || c->icem_cw_beta != o->noise_beta)) {
    if (!c->icem_cw) TRY(dalloc(c, &c->icem_cw, cwh.size()));
    c->icem_cw_host = cwh;
    c->icem_cw_beta = o->noise_beta;
    HIP_TRY(hipMemcpyAsync(c->icem_cw, c->icem_cw_host.data(), cwh.size() * sizeof(float), hipMemcpyHostToDevice, s));
  }
  // the kept rows ping-pong between two buffers of the call workspace (the update reads the old rows while it writes
  // the new ones); the first iteration reads keep_io, the last one writes it.  With one iteration both are keep_io:
  // its rows are copied aside first.
  float* W[2] = {nullptr, nullptr};
  const bool aside = K == 1 && o->carry_in > 0;
  if (nk > 0 && (K >= 2 || aside)) {
    TRY(c->cw.save.grow(c, 2 * keep_floats));
    W[0] = c->cw.save.p;
    W[1] = W[0] + keep_floats;
  }
  if (aside) HIP_TRY(hipMemcpyAsync(W[0], keep_io, keep_floats * sizeof(float), hipMemcpyDeviceToDevice, s));
  IcemRollArgs r;
  memset(&r, 0, sizeof(r));
  r.c = sampled_roll_args(c, B, N, x0, goal, mean_io, std_io, u_lo, u_hi);
  r.c.rng = gmpc_sampled_rng(o->seed, 0, 0.f);
  r.c.costs = cost_buf;
  r.ldc = ldc;
  r.p.nkeep = nk; r.p.white = white; r.p.cw = white ? nullptr : c->icem_cw;
  IcemUpdArgs u;
  memset(&u, 0, sizeof(u));
  u.B = B; u.E = o->num_elites; u.T = T; u.m = m; u.ldc = ldc;
  u.costs = cost_buf; u.lo = u_lo; u.hi = u_hi; u.mean = mean_io; u.sd = std_io;
  u.gamma = o->evolution_smoothing;
  u.best_U = best_U_io; u.best_cost = best_cost_io; u.U_out = U_out; u.return_best = o->return_best != 0;
  const float* keep_src = aside ? W[0] : keep_io;
  for (int i = 0; i < K; ++i) {
    const bool last = i == K - 1;
    r.c.rng.it = (uint32_t)(o->iter_offset + i);
    r.c.samples = last ? samples : nullptr;
    r.p.Nit = Nit[i];
    r.p.carry = i == 0 ? o->carry_in : nk;
    r.p.addmean = o->add_mean && last;
    r.p.keep = r.p.carry > 0 ? keep_src : nullptr;
    u.p = r.p;
    u.rng = r.c.rng;
    u.elites = last ? elites : nullptr;
    u.last = last;
    u.keep_out = nk == 0 ? nullptr : last ? keep_io : W[i & 1];
    if (launch_sampled_rows(c, r, s) || gmpc_launch_icem_update(u, s))
      return fail(GMPC_EINVAL, "icem: shape not covered");
    keep_src = u.keep_out;
  }
  // without an iteration nothing was sampled: the returned sequence is the mean
  if (K == 0 && U_out) HIP_TRY(hipMemcpyAsync(U_out, mean_io, BTm * sizeof(float), hipMemcpyDeviceToDevice, s));
  return sampled_finish(c, "icem", r.c, U_out ? U_out : mean_io, X, obj, s);
}
