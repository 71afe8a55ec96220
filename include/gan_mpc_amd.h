/*
 * gan_mpc_amd.h -- C ABI of libgan_mpc_amd.so: the MI355X (gfx950) implementation of the
 * GAN-MPC inner loop of returaj/gan_mpc.
 *
 * The reference has no FFI: its boundary is a Python object protocol.  Each entry
 * point below names the reference function(s) whose arithmetic it replaces (paths relative to the
 * reference repository root); the gan_mpc_amd Python package rebuilds the reference's Python protocol on top of
 * these calls through ctypes (see INTEGRATION.md for the binding a maintainer would add).
 *
 * Conventions
 *  - Every buffer is caller-owned DEVICE memory, fp32, row-major, unless stated otherwise.
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls only enqueue
 *    work; nothing synchronises unless stated.
 *  - Return value: 0 on success, a negative GMPC_E* code on failure; gmpc_last_error() returns a
 *    thread-local description of the last failure.  No C++ exception crosses this ABI.
 *  - A gmpc_ctx belongs to one GPU and is thread-compatible (one caller at a time).
 *  - There is no CPU fallback: without a HIP device every compute entry point fails.
 *  - Ordering contract: gmpc_bilevel_grad(_cotangent) / gmpc_upper_loss differentiate the solution the ctx holds
 *    after a COMPLETED gmpc_ilqr_solve of the same batch size.  gmpc_set_params, gmpc_rollout_cost,
 *    gmpc_lqr_backward(_after_rollout) and a failed or new gmpc_ilqr_solve overwrite parts of that
 *    state and therefore drop it: a later gmpc_bilevel_grad / gmpc_upper_loss fails with GMPC_EINVAL
 *    ("must precede") instead of differentiating a stale linearisation.  gmpc_rollout_vjp, gmpc_expert_vjp,
 *    gmpc_critic_vjp, gmpc_critic_dir_vjp, gmpc_cem_solve, gmpc_icem_solve and gmpc_mppi_solve drop nothing: they may run between a
 *    solve and its bilevel calls, or between a bilevel call and gmpc_bilevel_grad_inputs / _dynamics.  gmpc_mppi_vjp
 *    rolls its samples out through the ctx's buffers and drops a held solution, as gmpc_rollout_cost does.
 *
 * Parameter layouts (flat fp32 vectors, flax Dense order: kernel (in,out) row-major, then bias):
 *   dyn    : for l in 0..dyn_layers-1:  W_l[dims[l]][dims[l+1]], b_l[dims[l+1]]
 *            dims[0] = n+m, dims[last] = n          (reference dynamics/nn.py:27-34)
 *   cost   : same, dims[0] = n, dims[last] = fout   (reference cost/nn.py:23-29)
 *   mpc_w  : 3 raw weights (action, state, terminal) (reference gan/runner.py:41, cost_model.py:37)
 *   critic : Wx[n][4F], Wh[F][4F], b[4F] (gate order i,f,g,o), then the head's Dense layers
 *            head_dims[0] = F, head_dims[last] = 1   (reference critic/nn.py:28-42)
 */
#ifndef GAN_MPC_AMD_H
#define GAN_MPC_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

#define GMPC_MAX_LAYERS 8
#define GMPC_PROF_SLOTS 10

enum {
  GMPC_OK = 0,
  GMPC_EINVAL = -1,      /* bad argument / unsupported shape */
  GMPC_ENODEV = -2,      /* no usable HIP device */
  GMPC_EHIP = -3,        /* a HIP runtime call failed */
  GMPC_ENOMEM = -4
};

typedef struct gmpc_ctx gmpc_ctx;

typedef struct gmpc_shape {
  int n;                /* state size (xc size; the MLP dynamics has an empty carry) */
  int m;                /* action size */
  int T;                /* horizon H */
  int dyn_layers;       /* number of Dense layers of the dynamics MLP */
  int dyn_dims[GMPC_MAX_LAYERS + 1];
  int cost_layers;
  int cost_dims[GMPC_MAX_LAYERS + 1];
  int lstm_features;    /* F */
  int head_layers;      /* Dense layers after the LSTM (>= 1, last one has 1 output) */
  int head_dims[GMPC_MAX_LAYERS + 1];
  /* LSTM dynamics variant (reference dynamics/nn.py:37-57; 0 = the MLP variant, the yaml default):
   * xc = [x (x_size), c (F), h (F)], n = x_size + 2F, the cell runs on [x, u] and dyn_dims describes the
   * relu tail h' -> x: dyn_dims[0] = F, dyn_dims[last] = x_size.  Goals, desired sequences, the critic and
   * the expert model keep x_size columns; the cost MLP takes the whole xc (cost_dims[0] = n).
   * dyn vector: Wx[(x_size+m)][4F] | Wh[F][4F] | b[4F] (gates i,f,g,o) | the tail's Dense layers. */
  int dyn_lstm_features;
  int x_size;           /* 0 or n for the MLP dynamics */
} gmpc_shape;

/* trajax iLQR keyword set, reference policy/eval.py:10-20 */
typedef struct gmpc_ilqr_opts {
  int maxiter;
  float grad_norm_threshold;
  float relative_grad_norm_threshold;
  float obj_step_threshold;
  float inputs_step_threshold;
  int make_psd;          /* must be 0 (the reference never sets it) */
  float psd_delta;
  float alpha_0;
  float alpha_min;
} gmpc_ilqr_opts;

const char* gmpc_last_error(void);
const char* gmpc_version(void);

/* Sizes of the flat parameter vectors for a shape: which = 0 dyn, 1 cost, 2 critic. */
long gmpc_param_count(const gmpc_shape* shape, int which);

/* Flat layout of a parameter vector, leaf by leaf, so that a caller in any language can pack a flax
 * checkpoint (replaces the pytree plumbing of policy/eval.py:56-62, gan/js_policy.py:32-39 and the
 * Python-only packing of gan_mpc_amd/params.py).  Element (r, c) of a leaf lives at
 * flat[offset + r * ld + c]; names are flax tree paths ("params/Dense_0/kernel", critic:
 * "params/ScanOptimizedLSTMCell_0/ii/kernel" ... -- the per-gate LSTM kernels are column blocks of the
 * concatenated Wx / Wh, hence ld = 4F there).
 *   which = 0 dyn, 1 cost, 2 critic (the vectors gmpc_set_params / the critic calls take),
 *           3 the host package's training vector [mpc_weights | cost_params | dynamics_params | critic_params]
 * Writes at most max_leaves entries (leaves may be NULL with max_leaves 0 to size the buffer) and
 * returns the number of leaves, or a negative GMPC_E* code. */
typedef struct gmpc_leaf {
  char name[64];
  long offset;
  int rows, cols, ld;
} gmpc_leaf;
int gmpc_pack_layout(const gmpc_shape* shape, int which, gmpc_leaf* leaves, int max_leaves);

/* One context per GPU.  Allocates the workspace for up to max_batch trajectories
 * (and 2*max_batch critic sequences). */
int gmpc_create(const gmpc_shape* shape, int max_batch, int device, gmpc_ctx** out);
int gmpc_destroy(gmpc_ctx* ctx);

/* Bind the model parameters used by the trajectory kernels (device pointers; they must stay valid
 * and unchanged until the next gmpc_set_params).  Builds the transposed weight copies the backward
 * chains read.  Replaces the params-dict unwrapping of policy/eval.py:64-73. */
int gmpc_set_params(gmpc_ctx* ctx, const float* mpc_w, const float* dyn, const float* cost,
                    void* stream);

/* a1-a4,a7: X = rollout(dynamics, U, x0); costs[t] = get_cost(X[t], pad(U)[t], t).
 * Replaces trajax rollout/evaluate as called at policy/optimizers.py:24-31 with
 * dynamics/nn.py:27-34, cost/cost_model.py:20-42, cost/nn.py:23-29.
 *   x0 [B][n], U [B][T][m], goal [B][T+1][n]  ->  X [B][T+1][n], costs [B][T+1]            */
int gmpc_rollout_cost(gmpc_ctx* ctx, int B, const float* x0, const float* U, const float* goal,
                      float* X, float* costs, void* stream);

/* a4 as the model protocol calls it (base.py:4-9, cost/cost_model.py:33-42 get_cost(xc, u, t, ...)): the
 * cost of B independent (x, u) pairs outside a rollout.  terminal == 0: the staging branch with
 * goal_row [B][n] = goal_X[t]; terminal != 0: the terminal branch w2 |MLP(x)|^2 of an arbitrary state
 * (u, goal_row may be NULL).  x [B][n], u [B][m] -> cost [B]. */
int gmpc_get_cost(gmpc_ctx* ctx, int B, const float* x, const float* u, const float* goal_row,
                  int terminal, float* cost, void* stream);

/* a1-a2 as the model protocol calls it (base.py:15-22, dynamics/dynamics_model.py:45-48 predict(xc, u, t,
 * params)): next_x [B][n] = dynamics(x, u) for B independent pairs (a horizon-1 pass of the rollout
 * kernel; drops a held iLQR solution, see the ordering contract). */
int gmpc_predict(gmpc_ctx* ctx, int B, const float* x, const float* u, float* next_x, void* stream);

/* One iLQR backward pass at an arbitrary trajectory (X, U): linearise the dynamics (the relu sign
 * masks are recomputed from (X, U)), quadratise the cost, run the time-varying LQR (Riccati)
 * recursion and the adjoint recursion.
 * Replaces trajax linearize/quadratize/tvlqr/adjoint inside trajax ilqr (policy/optimizers.py:19,55).
 *   -> K [B][T][m][n], k [B][T][m], grad [B][T][m], adjoints [B][T+1][n]; any output may be NULL.
 *   AB (optional) [B][T][n][n+m]: rows of [A_t | B_t] = d f/d[x,u]. */
int gmpc_lqr_backward(gmpc_ctx* ctx, int B, const float* X, const float* U, const float* goal,
                      float* K, float* k, float* grad, float* adjoints, float* AB, void* stream);

/* Same as gmpc_lqr_backward, but reuses the relu sign masks that the immediately preceding
 * gmpc_rollout_cost of this ctx produced for exactly this (X, U): the fused rollout + backward
 * "step" of one iLQR iteration (what bench.py times). */
int gmpc_lqr_backward_after_rollout(gmpc_ctx* ctx, int B, const float* X, const float* U,
                                    const float* goal, float* K, float* k, float* grad,
                                    float* adjoints, float* AB, void* stream);

/* a6: full iLQR solve (policy/optimizers.py:10-21 -> trajax ilqr), one independent solve per
 * trajectory (the reference's jax.vmap axis, policy/base.py:122-125).
 *   U_init [B][T][m] -> X [B][T+1][n], U [B][T][m], obj [B], grad [B][T][m], adjoints [B][T+1][n],
 *   iterations [B] (int32).  Synchronises the stream before returning. */
int gmpc_ilqr_solve(gmpc_ctx* ctx, int B, const float* x0, const float* U_init, const float* goal,
                    const gmpc_ilqr_opts* opts, float* X, float* U, float* obj, float* grad,
                    float* adjoints, int* iterations, void* stream);

/* a6 in ONE kernel launch: the complete iLQR solve of every trajectory, one workgroup per trajectory from the first
 * rollout to the last iteration, no host round trip between iterations (the short-horizon / batch-1 MPC action regime:
 * policy/eval.py:126-128 runs one solve per control step).  Same arguments and results as gmpc_ilqr_solve (the line
 * search evaluates its halvings in groups and accepts the first decrease in halving order, as the sequential loop
 * does); asynchronous on `stream`: nothing is synchronised, no host-built vectors.
 * Coverage -- checked before any launch, anything else fails with GMPC_EINVAL ("fused ..."):
 *   MLP dynamics only (dyn_lstm_features == 0); n <= 64 and m <= 32; T <= 32; at most 16 step sizes
 *   alpha_0 / 2^k above alpha_min (the reference's 1 / 5e-5 needs 15); make_psd refused as by gmpc_ilqr_solve.
 *   Every hidden width and cost fout the ctx accepts.
 * ctx state left behind, as after gmpc_ilqr_solve: X, U, goals, obj, grad, adjoints; [A|B] of the final linearisation
 * (gmpc_debug_buffer 5, [B][T][n][n+m]); the terminal quadratisation; K / k (6 / 7); alpha / obj_step / U_step
 * (8 / 9 / 10); the held batch size -- gmpc_bilevel_grad / gmpc_upper_loss may follow on the same stream.  The relu masks
 * of gmpc_rollout_cost, the line-search work lists and counters (gmpc_linesearch_candidates / _stats, debug buffers 12
 * / 13) still describe the last round-based solve. */
int gmpc_ilqr_solve_fused(gmpc_ctx* ctx, int B, const float* x0, const float* U_init, const float* goal,
                          const gmpc_ilqr_opts* opts, float* X, float* U, float* obj, float* grad,
                          float* adjoints, int* iterations, void* stream);

/* Control-limited iLQR in one kernel launch: gmpc_ilqr_solve_fused under box bounds u_lo <= u_t <= u_hi on the
 * controls (control-limited DDP, Tassa, Mansard and Todorov 2014).  u_lo, u_hi: device pointers, [m] each,
 * shared by all trajectories and steps; either may be NULL (unbounded on that side), entries may be -inf / +inf.  The
 * caller guarantees u_lo <= u_hi and no NaN entry (the pointers are device memory: not checked here).
 *   The start is clamped, every candidate rollout applies u = clamp(U_t + (alpha k_t + K_t (x - X_t))), and the gains of
 *   a step are those of the box QP  min 1/2 y^T G y + h^T y,  u_lo - u_t <= y <= u_hi - u_t  (projected Newton, at most
 *   40 iterations): k_t = y, the rows of K_t of clamped controls are exactly 0.  The continuation test uses the norm of
 *   the projected gradient; `grad` is the full gradient (its entries at clamped controls are the bounds' multipliers).
 *   With no bound active every result is bit for bit that of gmpc_ilqr_solve_fused.
 * Arguments, results, coverage and asynchrony as gmpc_ilqr_solve_fused; refusals start with "box solve: ...".
 * ctx state left behind: X, U, goals, obj, grad, adjoints, [A|B], K / k, alpha / obj_step / U_step as after the fused
 * solve, and gmpc_debug_buffer 15 ([B][2]: QPs of the solve that stopped at the iteration cap, QP iterations of the
 * solve), 16 ([B][T]: QP iterations per step of the last backward pass), 17 ([B][T][m]: 1.0 where a control is in the
 * final clamped set of that pass).
 * NO solution is held for the bilevel tail: gmpc_bilevel_grad*, gmpc_upper_loss after this call fail with "must
 * precede" (the MPC action path does not pay for the clamped-set launch).  gmpc_ilqr_solve_box_held is the variant
 * they may follow. */
int gmpc_ilqr_solve_box(gmpc_ctx* ctx, int B, const float* x0, const float* U_init, const float* goal,
                        const gmpc_ilqr_opts* opts, float* X, float* U, float* obj, float* grad,
                        float* adjoints, int* iterations, void* stream, const float* u_lo, const float* u_hi);

/* gmpc_ilqr_solve_box with the solution held for the bilevel tail: signature, results, coverage and
 * refusals are gmpc_ilqr_solve_box's (the same kernel launch), then one small kernel on the same stream builds the
 * clamped set of the solution from the ctx's U and grad and the caller's u_lo / u_hi (NULL: unbounded on that side):
 *   C = {(t, j) : (U_tj == lo_j and grad_tj > 0) or (U_tj == hi_j and grad_tj < 0)},  exact fp32 comparisons,
 * the entries the solve's continuation test leaves out of its projected-gradient norm (a NaN compares false: free).
 * It is kept as gmpc_debug_buffer 18: [B][T] 32-bit words, bit j = control j clamped (m <= 32 on this path).
 * gmpc_bilevel_grad, gmpc_bilevel_grad_cotangent, gmpc_bilevel_grad_inputs, gmpc_bilevel_grad_dynamics and
 * gmpc_upper_loss may follow with their usual arguments.  They differentiate through the active set held fixed: the
 * clamped controls sit on bounds that depend on no parameter and the free gradient vanishes, so the implicit-function
 * formula is unchanged with the masked solve H_C = 0, H_F = A_FF^-1 Bvec_F (A = d^2 J / dU^2) and dX the tangent roll
 * of H.  Debug buffers 2 / 3 / 4 keep their meaning (2: the masked H).  With no bound active the tail's results are
 * bit for bit those after gmpc_ilqr_solve_fused.  Gradients with respect to the bounds themselves are not computed.
 * Any later solve, gmpc_set_params or call that drops a held solution drops this one. */
int gmpc_ilqr_solve_box_held(gmpc_ctx* ctx, int B, const float* x0, const float* U_init, const float* goal,
                             const gmpc_ilqr_opts* opts, float* X, float* U, float* obj, float* grad,
                             float* adjoints, int* iterations, void* stream, const float* u_lo, const float* u_hi);

/* Test hook, host memory only, no ctx and no device: ONE box QP of gmpc_ilqr_solve_box's backward pass, solved on the
 * host by the routine the kernel runs on one lane (the same source compiled for the host).  G [m][m] symmetric WITHOUT
 * the 1e-8 regulariser (the routine adds it), h, u, u_lo, u_hi [m]; m <= 32.  -> y [m] (the minimiser of
 * 1/2 y^T (G + 1e-8 I) y + h^T y on u_lo - u <= y <= u_hi - u), clamped [m] (1 / 0: the final clamped set),
 * iterations [2]: the QP iterations and 1 where it stopped at a cap.  Returns 0, or GMPC_EINVAL. */
int gmpc_box_qp_host(int m, const float* G, const float* h, const float* u, const float* u_lo,
                     const float* u_hi, float* y, int* clamped, int* iterations);

/* The cross-entropy method on the same cost and dynamics (trajax `cem`, the sampling solver beside `ilqr`; DESIGN
 * §20): control limits by construction, at any horizon, no Jacobian and no Riccati sweep.  Per problem b and
 * iteration it = iter_offset + i, i < max_iter:
 *   z[s][t][j] standard normal from Philox4x32-10, key (seed low word, seed high word), counter (e >> 2, s, b, it)
 *   and output word e & 3 for e = t m + j; words become u = ((r >> 9) 2 + 1) 2^-24 and Box-Muller pairs (u0, u1),
 *   (u2, u3) give z = sqrt(-2 ln u0) (cos, sin)(2 pi u1);  smoothing along time zt_0 = z_0,
 *   zt_t = beta zt_{t-1} + sqrt(1 - beta^2) z_t (beta = sampling_smoothing);
 *   u = clamp(std_tj zt + mean_tj, lo_j, hi_j)  (a NaN stays a NaN);  cost_s = the objective of gmpc_rollout_cost under
 *   the sample's controls (fp32 sum over t, terminal cost last);  the num_elites smallest by (cost, sample index), a
 *   NaN cost counting as +inf, give new_mean = sum u / E and new_std = sqrt(sum (u - new_mean)^2 / E) in rank order;
 *   mean <- gamma mean + (1 - gamma) new_mean, std likewise (gamma = evolution_smoothing).
 * mean_io / std_io [B][T][m] hold the initial mean and std and receive the final ones (the mean is trajax' U: not
 * clipped).  u_lo / u_hi: device [m] shared by all problems and steps, either may be NULL (unbounded on that side).
 * X [B][T+1][n] and obj [B]: the rollout and objective of the final mean (either may be NULL).  costs [B][N],
 * elites [B][E] (sample indices in rank order) and samples [B][N][T][m]: those of the last iteration, each may be NULL
 * (nothing of size B N T m exists unless `samples` is passed).  One call with max_iter = K equals K chained calls with
 * max_iter = 1 and iter_offset = 0 .. K-1, bit for bit; a sample's cost depends on neither N nor B.
 * Coverage -- anything else fails with GMPC_EINVAL ("cem: ...") before any launch: MLP dynamics
 * (dyn_lstm_features == 0); every dynamics and cost width <= 256 and n + m <= 256; any T; B <= max_batch;
 * 1 <= num_elites <= num_samples <= 4096; max_iter >= 0; 0 <= sampling_smoothing < 1 (above 0 the sampler costs
 * O(T) per control); 0 <= evolution_smoothing <= 1.
 * 2 max_iter + 1 launches on `stream` (2 max_iter with X and obj both NULL), no host synchronisation, no atomics;
 * deterministic.  Stateless like gmpc_rollout_vjp: it writes the caller's arrays and the call workspace only (B N
 * floats when costs is NULL, allocated by the first call that needs more than the ctx holds), touches neither the
 * ctx's trajectories and masks nor a held solution. */
typedef struct gmpc_cem_opts {
  int max_iter, num_samples, num_elites, iter_offset;
  float sampling_smoothing, evolution_smoothing;
  unsigned long long seed;
} gmpc_cem_opts;
int gmpc_cem_solve(gmpc_ctx* ctx, int B, const float* x0, const float* goal,
                   const float* u_lo, const float* u_hi,
                   const gmpc_cem_opts* opts, float* mean_io, float* std_io,
                   float* X, float* obj,
                   float* costs, int* elites, float* samples,
                   void* stream);

/* Model-predictive path integral control on the same samples: gmpc_cem_solve with the elite cut replaced
 * by softmax weights, so that the update is a smooth function of the sample costs (gmpc_mppi_vjp differentiates it).
 * Per problem b and iteration it = iter_offset + i, i < max_iter: samples u_s and costs J_s exactly as gmpc_cem_solve
 * forms them (same Philox counters, smoothing and clamp, same kernel); then
 *   w_s = exp(-(J_s - J_min) / temperature), J_min over the finite costs, w_s = 0 for a NaN or infinite cost;
 *   new_mean = sum_s w_s u_s / sum_s w_s (fp32, both sums in sample order, whatever B and the launch geometry);
 *   mean <- gamma mean + (1 - gamma) new_mean (gamma = evolution_smoothing).
 * A problem without a finite cost keeps its mean, bit for bit.  std [B][T][m] is read and never written (classic
 * MPPI: the sampling distribution's width is fixed).  mean_io, u_lo / u_hi, X and obj as for gmpc_cem_solve.
 * costs [B][N], weights [B][N] (normalised: w_s / sum w) and samples [B][N][T][m]: those of the last iteration, each
 * may be NULL.  means_trace [max_iter][B][T][m]: the mean BEFORE each iteration; costs_trace [max_iter][B][N]: the
 * costs of each iteration; each may be NULL (gmpc_mppi_vjp needs both).  One call with max_iter = K equals K chained
 * calls with max_iter = 1 and iter_offset = 0 .. K-1, bit for bit, and the traces are the chained calls' inputs and
 * costs.
 * Coverage -- anything else fails with GMPC_EINVAL ("mppi: ...") before any launch: as gmpc_cem_solve without the
 * elites, and temperature > 0 and finite.
 * 2 max_iter + 1 launches on `stream` (2 max_iter with X and obj both NULL), no host synchronisation, no atomics;
 * deterministic; stateless like gmpc_cem_solve (B N floats of call workspace when costs and costs_trace are NULL). */
typedef struct gmpc_mppi_opts {
  int max_iter, num_samples, iter_offset;
  float sampling_smoothing, evolution_smoothing, temperature;
  unsigned long long seed;
} gmpc_mppi_opts;
int gmpc_mppi_solve(gmpc_ctx* ctx, int B, const float* x0, const float* goal,
                    const float* u_lo, const float* u_hi,
                    const gmpc_mppi_opts* opts, float* mean_io, const float* std,
                    float* X, float* obj,
                    float* costs, float* weights, float* samples,
                    float* means_trace, float* costs_trace,
                    void* stream);

/* The VJP of gmpc_mppi_solve: the true derivative of (U, X, obj) = (final mean, its rollout, its objective) w.r.t. x0,
 * the initial mean, the goals and the parameters, through the sampler (the normals are constants; the clamp passes a
 * cotangent where the unclamped control lies strictly inside the bounds).  x0 .. std and opts: the forward call's;
 * means_trace / costs_trace: what it wrote; U [B][T][m], X [B][T+1][n]: its final mean and rollout.  Cotangents
 * gU [B][T][m], gX [B][T+1][n], gobj [B]: any may be NULL, not all.
 *   -> grad_x0 [B][n], grad_Uinit [B][T][m], grad_goal [B][T+1][n] per problem; grad_theta_sum / grad_dyn_sum in
 *   gmpc_rollout_vjp's layouts, SUMMED over the batch.  Any may be NULL, not all.
 * g = gU + the gmpc_rollout_vjp of the final rollout under gX and gobj (on every cost of the row); then for
 * k = max_iter - 1 .. 0, with w~ = w / sum w and new_mean = sum w~_s u_s of iteration k:
 *   a_s = <g, u_s - new_mean>,  c_s = -(1 - gamma) / temperature  w~_s a_s: the cotangent of every cost of sample s;
 *   the rollout VJP of the N sample rows under c gives GU_s, Gx0_s, Ggoal_s and the parameter sums;
 *   g <- gamma g + sum_s mask_s ((1 - gamma) w~_s g + GU_s);  grad_x0 += sum_s Gx0_s, grad_goal likewise.
 * grad_Uinit is the final g.  The sample rows run in chunks of floor(max_batch / num_samples) problems; every sum has a
 * fixed order (samples, then chunks, then iterations): deterministic, no atomics.  A problem whose iteration had no
 * finite cost passes g through that iteration (its NaN states still reach the sums over the batch, as NaN rows do in
 * gmpc_rollout_vjp: grad_theta_sum and grad_dyn_sum are then NaN).
 * Refusals (GMPC_EINVAL, "mppi: ...", before any launch): those of gmpc_mppi_solve; num_samples > max_batch; NULL
 * traces with max_iter > 0; every cotangent or every output NULL.
 * Ordering contract: like gmpc_rollout_cost, the sample rollouts overwrite the ctx's relu masks and objectives, so the
 * call DROPS a solution held by the ctx (run it on a second context beside a solve whose bilevel calls are pending).
 * Workspace, allocated by the first call that needs more than the ctx holds (a synchronising hipMalloc) and kept: with
 * R = min(B, floor(max_batch / N)) N rows, R (2 T m + 3 (T + 1) n + 2 n + T + 2) + B (T m + T + 1) floats plus one
 * copy of each parameter sum, beside gmpc_rollout_vjp's own workspace for R rows. */
int gmpc_mppi_vjp(gmpc_ctx* ctx, int B, const float* x0, const float* goal,
                  const float* u_lo, const float* u_hi,
                  const gmpc_mppi_opts* opts, const float* std,
                  const float* means_trace, const float* costs_trace,
                  const float* U, const float* X,
                  const float* gU, const float* gX, const float* gobj,
                  float* grad_x0, float* grad_Uinit, float* grad_goal,
                  float* grad_theta_sum, float* grad_dyn_sum, void* stream);

/* The sample-efficient cross-entropy method (iCEM: Pinneri et al., CoRL 2020) on gmpc_cem_solve's sampler,
 * rollout and sort: coloured noise along the horizon, elites kept from one iteration (and one MPC step) to the next, a
 * sample count that shrinks per iteration, the mean as a candidate in the last iteration, the best row seen returned.
 * Per problem b and iteration it = iter_offset + i, i < max_iter, a pool of R_it = N_it + c_it + a_it rows:
 *   rows 0 .. N_it-1   fresh: u = clamp(std zt + mean) with gmpc_cem_solve's Philox counters for sample index = row.
 *     noise_beta == 0 or T < 2: zt = z, the control is gmpc_cem_solve's at sampling_smoothing 0, bit for bit.  Otherwise
 *     with z_k the normal e = k m + j of the row (k < T) and cw the weights below, in fp32 fma, k ascending,
 *       zt_t = cw_0 z_0 + sum_{1<=k, 2k<T} cw_k (z_{2k-1} cos(2 pi k t / T) + z_{2k} sin(2 pi k t / T))
 *              + [T even] cw_{T/2} z_{T-1} (-1)^t,   the angle as cospi / sinpi of 2 ((k t) mod T) / T;
 *     w_k = (k / T)^(-noise_beta / 2), w_0 = w_1;  cw_0 = w_0 / s, cw_k = sqrt(2) w_k / s (2k < T), cw_{T/2} = w_{T/2} / s;
 *     s^2 = w_0^2 + 2 sum_{2k<T} w_k^2 + [T even] w_{T/2}^2 (float64 on the host, rounded to fp32): unit variance at
 *     every step, power spectrum ~ f^-noise_beta;
 *   rows N_it .. N_it+c_it-1   carried: the first c_it rows of the keep buffer [B][num_keep][T][m], clamped; c_it =
 *     carry_in in the call's first iteration, num_keep afterwards;
 *   a_it = 1 iff add_mean and i == max_iter - 1: the row clamp(mean).
 *   N_it = max(floor(n_it), min(N, 2 E)) with n_0 = N, n_{k+1} = n_k / decay in float64.
 * Every row is rolled out and costed as gmpc_cem_solve's samples are (carried rows again: nothing is cached).  The E
 * smallest by (cost, pool row), NaN as +inf, refit mean and std as in gmpc_cem_solve (sums in rank order, gamma =
 * evolution_smoothing); a problem without a finite cost keeps its mean and std, bit for bit.  The controls of ranks
 * 0 .. num_keep-1 become the keep buffer; where the rank-0 cost is strictly below best_cost_io[b] (never for a NaN),
 * best_cost_io[b] and best_U_io[b] take that row's cost and controls -- initialise best_cost_io to +inf.
 * mean_io / std_io [B][T][m], u_lo / u_hi as for gmpc_cem_solve.  keep_io: in, its first carry_in rows; out, the last
 * iteration's kept rows (may be NULL with num_keep 0).  best_U_io [B][T][m] / best_cost_io [B]: both or neither.
 * U_out [B][T][m] (may be NULL without return_best): best_U where return_best is set and the best cost is finite, the
 * final mean otherwise (and with max_iter 0); X [B][T+1][n], obj [B]: its rollout and objective, no clamp (either may
 * be NULL; the mean's when U_out is NULL).  costs [B][N+num_keep+1] (the first R of the last iteration), elites [B][E]
 * (pool rows in rank order), samples [B][N][T][m] (the fresh rows of the last iteration, its first N_it): each may be
 * NULL.  One call of K iterations equals K chained calls of one (carry_in = num_keep and iter_offset = 1 .. K-1 after
 * the first, add_mean in the last only), bit for bit.  With num_keep = carry_in = 0, decay = 1, noise_beta = 0,
 * add_mean = return_best = 0: mean, std, X, obj, costs and elites are gmpc_cem_solve's at sampling_smoothing 0, bit
 * for bit.
 * Refused with GMPC_EINVAL ("icem: ...") before any launch: gmpc_cem_solve's shape coverage; 1 <= num_elites <=
 * num_samples; 0 <= carry_in <= num_keep <= num_elites; num_samples + num_keep + 1 <= 4096; max_iter, iter_offset >= 0;
 * decay >= 1, noise_beta >= 0, both finite; 0 <= evolution_smoothing <= 1; keep_io NULL with num_keep > 0; best_*_io
 * or U_out NULL with return_best.
 * 2 max_iter + 1 launches on `stream` (2 max_iter with X and obj NULL), no atomics, no host synchronisation;
 * deterministic; stateless like gmpc_cem_solve.  Call workspace (grown by the first call that needs more): B (N +
 * num_keep + 1) floats when costs is NULL, two keep buffers; the T/2 + 1 weights are uploaded when noise_beta changes;
 * a one-iteration call with carry_in > 0 copies keep_io aside first (device to device, on `stream`).
 * gmpc_icem_plan_host (host only, no ctx): N_it [max_iter] and cw [T/2 + 1] of the options, either may be NULL; the
 * same refusals of the options. */
typedef struct gmpc_icem_opts {
  int max_iter, num_samples, num_elites, num_keep, carry_in, iter_offset, add_mean, return_best;
  float noise_beta, evolution_smoothing, decay;
  unsigned long long seed;
} gmpc_icem_opts;
int gmpc_icem_solve(gmpc_ctx* ctx, int B, const float* x0, const float* goal,
                    const float* u_lo, const float* u_hi,
                    const gmpc_icem_opts* opts, float* mean_io, float* std_io, float* keep_io,
                    float* best_U_io, float* best_cost_io, float* U_out,
                    float* X, float* obj,
                    float* costs, int* elites, float* samples,
                    void* stream);
int gmpc_icem_plan_host(const gmpc_icem_opts* opts, int T, int* N_it, float* cw);

/* The operand precision of the sampling solvers' sampled rollouts: a property of the context, fp32 until set.  No
 * stream, no device work; any other value is GMPC_EINVAL ("sampled precision: ...").
 *   GMPC_SAMPLED_BF16: every launch of gmpc_cem_solve / gmpc_mppi_solve / gmpc_icem_solve that rolls out SAMPLED rows
 *   runs the dynamics and cost layers on v_mfma_f32_16x16x32_bf16: the weight matrices rounded once to bf16 (to nearest
 *   even; biases stay fp32), every layer input ([x_t; u_t], the relu outputs, x_T) rounded to bf16 when it becomes a
 *   matrix operand, products accumulated in fp32; the bias add, the relu, the residual x += out + b (the states stay
 *   fp32 across steps), the controls, the stage cost (fp32 x_t, u_t, goal) and the terminal w2 |y|^2 (the fp32,
 *   unrounded output of the last cost layer) are what they are in fp32 mode.  `samples` is bitwise the fp32 mode's;
 *   `costs` (and so the elites, the weights and iCEM's best_cost_io) are the bf16-mode costs.  The returned sequence's
 *   own rollout always runs in fp32: X and obj are those of the true model at the returned controls in either mode.
 *   The bf16 weight image is built by the first bf16-mode solve after a gmpc_set_params, on that solve's stream
 *   (gmpc_set_params only marks it stale): weights changed in place need a gmpc_set_params, as for every other derived
 *   copy.  gmpc_mppi_vjp is the derivative of the fp32 solve and is refused in bf16 mode ("mppi vjp: fp32 sampled
 *   rollouts only").  Coverage and refusals are those of fp32 mode. */
enum { GMPC_SAMPLED_FP32 = 0, GMPC_SAMPLED_BF16 = 1 };
int gmpc_set_sampled_precision(gmpc_ctx* ctx, int precision);

/* A dynamics ensemble under the sampling solvers' sampled rollouts: a property of the context,
 * off until set.  dyn_members: device, [P][dyn_param_count], each row a dynamics parameter vector in the layout of the
 * `dyn` argument of gmpc_set_params; kept, not owned.  1 <= P <= 16; P == 0 (any pointer) switches the ensemble off;
 * every call, also with the same pointer, means "the members changed".  No stream, no device work.  GMPC_EINVAL
 * ("ensemble: ...") for a null ctx, P outside [0, 16], a null pointer with P > 0, and a context the sampling solvers
 * refuse (LSTM dynamics, a width above 256).  gmpc_set_params neither drops nor changes the ensemble.
 *   While set, every launch of gmpc_cem_solve / gmpc_mppi_solve / gmpc_icem_solve that rolls out SAMPLED rows rolls
 *   each row out once per member p, under member p's dynamics weights and biases (the cost MLP, mpc_w, x0, the goals
 *   and the controls are shared): J_p, the arithmetic of a solve without an ensemble.  The row's cost is (in the
 *   default mode; gmpc_set_sampled_ensemble_mode below has the others)
 *   (((J_0 + J_1) + J_2) + ... + J_{P-1}) * (1.0f / (float)P) in fp32 (a NaN J_p makes it NaN), and everything that
 *   reads costs -- elites, weights, kept rows, iCEM's best row and best_cost_io, `costs` / `costs_trace` -- reads that.
 *   `samples` is bitwise that of a solve without an ensemble.  X and obj of the returned sequence stay on the
 *   context's own dynamics (the nominal model).  In bf16 mode each member's weight matrices are rounded to bf16 images
 *   by the first bf16-mode solve after this call, on that solve's stream; members changed in place need this call
 *   again.  gmpc_mppi_vjp differentiates the nominal model only and is refused while an ensemble is set ("mppi vjp:
 *   ..."). */
int gmpc_set_sampled_ensemble(gmpc_ctx* ctx, int P, const float* dyn_members);

/* What the sampling solvers do with a set ensemble: a property of the context, like the precision
 * and the ensemble; the default is {GMPC_ENS_MEAN, 0, GMPC_ENS_FIXED, 0}, the rule above.  No stream, no device work.
 * Independent of the members: gmpc_set_sampled_ensemble and gmpc_set_params neither reset nor change it, it may be set
 * before an ensemble is, and it has no effect while none is set.
 *   propagation  GMPC_ENS_FIXED: cost plane q is member q, Q = P planes (particles must be 0).
 *                GMPC_ENS_TS1:   Q = particles planes, 1 <= particles <= 16; particle q at step t of iteration `it`
 *                                runs under member umulhi(philox4x32_10(counter (t, q, 0xFFFFFFFF, it), key (seed low
 *                                word, seed high word))[0], P), `it` the solve's iter_offset + i.  The schedule is
 *                                shared by every row and problem: the rows of an iteration are ranked under the same
 *                                model sequences (common random numbers).
 *   aggregate    over the planes' costs J_0 .. J_{Q-1} of a row, every operation one IEEE fp32 operation in ascending
 *                q, invQ = 1.0f / (float)Q:
 *                GMPC_ENS_MEAN      (((J_0 + J_1) + ...) + J_{Q-1}) * invQ
 *                GMPC_ENS_MEAN_STD  mean + risk * sqrt(ss * invQ), ss = (((0 + d_0 d_0) + d_1 d_1) + ...), d_q = J_q -
 *                                   mean; risk < 0 is optimism
 *                GMPC_ENS_MAX       w = J_0; w = (J_q > w || J_q != J_q) ? J_q : w
 *                A NaN J_q makes the cost NaN in every mode.
 * `samples`, X and obj are as under gmpc_set_sampled_ensemble; gmpc_mppi_vjp stays refused while an ensemble is set.
 * GMPC_EINVAL ("ensemble mode: ...", the mode left as it was) for a null ctx or mode, an aggregate outside 0..2, a
 * propagation outside 0..1, a non-finite risk, risk != 0 with an aggregate other than GMPC_ENS_MEAN_STD, particles != 0
 * with GMPC_ENS_FIXED, and particles outside [1, 16] with GMPC_ENS_TS1. */
enum { GMPC_ENS_MEAN = 0, GMPC_ENS_MEAN_STD = 1, GMPC_ENS_MAX = 2 };   /* aggregate   */
enum { GMPC_ENS_FIXED = 0, GMPC_ENS_TS1 = 1 };                         /* propagation */
typedef struct { int aggregate; float risk; int propagation; int particles; } gmpc_ensemble_mode;
int gmpc_set_sampled_ensemble_mode(gmpc_ctx* ctx, const gmpc_ensemble_mode* mode);

/* A plan's rollout under every member of a dynamics ensemble, and the members' spread: B
 * problems, each with its own initial state, goals and controls, rolled S steps under each of the P members in one
 * launch; forward only.
 *   dyn_members [P][dyn_param_count]: the layout of gmpc_set_sampled_ensemble, passed per call (nothing is kept)
 *   x0 [B][n], U [B][S][m], 1 <= S <= T, 1 <= B <= max_batch, 1 <= P <= 16
 *   goal [B][T+1][n] or NULL: NULL skips the cost terms and the cost MLP
 *   -> X      [P][B][S+1][n]  member p's states, X[p][b][0] = x0[b]
 *      costs  [P][B][T+1]     stage costs w0 (sqrt(|u_t|^2 + a^2) - a) + w1 (sqrt(|x_t - goal_t|^2 + a^2) - a), t < T, and
 *                             the terminal cost w2 |MLP_c(x_T)|^2 at t = T
 *      obj    [P][B]          their fp32 sum, t ascending, the terminal cost last
 *      x_mean [B][S+1][n]     (sum_p x_p) / P, the sum sequential in ascending p
 *      x_var  [B][S+1][n]     (sum_p (x_p - x_mean)^2) / P, the population variance, summed likewise
 *   each output may be NULL, not all of them; costs and obj need goal and S == T.
 * The arithmetic of a row is that of the sampling solvers' rollout: X[p] and obj[p] are bitwise what gmpc_cem_solve
 * with max_iter = 0 returns for U on a context whose bound dynamics are member p, and they depend on neither B, the
 * problem's place in the batch, nor P.  A non-finite member makes its own planes and the moments non-finite and leaves
 * the other members' planes as they are.
 * Stateless: mpc_w and the cost MLP come from the parameters bound by gmpc_set_params; a set sampled ensemble, its
 * mode, the sampled precision and a held solution are neither read nor changed.  Asynchronous on `stream` (two
 * launches at most), deterministic.  With moments but no X the members' planes live in the call workspace, grown (a
 * synchronising hipMalloc) by the first call that needs more.  Every refusal is GMPC_EINVAL with a message starting
 * "ensemble rollout: ", before any launch: a null ctx, dyn_members, x0 or U; B, S or P out of range; parameters not
 * set; every output NULL; costs or obj with goal == NULL or S != T; LSTM dynamics, a width or n + m above 256. */
int gmpc_ensemble_rollout(gmpc_ctx* ctx, int B, int S, int P, const float* dyn_members, const float* x0,
                          const float* U, const float* goal, float* X, float* costs, float* obj, float* x_mean,
                          float* x_var, void* stream);

/* The same rollout in closed loop: a reference trajectory tracked with its own time-varying
 * feedback gains under every member, in one member-parallel launch; forward only.  Per member p and problem b, with
 * x_0 = x0[b]:
 *   du_j    = sum_c K[b][t][j][c] (x_t[c] - X_ref[b][t][c])     one fmaf per c, c ascending, from 0
 *   du_j   += alpha * k[b][t][j]                                only with k; the product rounded first
 *   u_t     = clamp(U_ref[b][t] + du, u_lo, u_hi)               the clamp only with bounds; a NaN control stays NaN
 *   x_{t+1} = x_t + MLP_p([x_t; u_t])
 *   dyn_members, B, S, P, goal as for gmpc_ensemble_rollout
 *   x0 [B][n] or NULL: then X_ref[b][0]
 *   X_ref [B][S+1][n], U_ref [B][S][m]: the reference trajectory; K [B][S][m][n]: the gains, gmpc_lqr_backward's layout
 *   k [B][S][m] or NULL: no feed-forward term (alpha is then only checked)
 *   u_lo, u_hi [m] device vectors, both or neither (NULL: no clamp); u_lo <= u_hi is the caller's to keep
 *   -> X [P][B][S+1][n], costs [P][B][T+1], obj [P][B], x_mean, x_var [B][S+1][n] as gmpc_ensemble_rollout's, the costs
 *      on the applied controls
 *      U [P][B][S][m]  the applied controls, which differ per member
 *   each output may be NULL, not all of them; costs and obj need goal and S == T.
 * The dynamics' and the costs' arithmetic is gmpc_ensemble_rollout's own: with K = 0, no k and no bounds X, costs, obj
 * and the moments are bitwise that call's for U = U_ref, and a member that reproduces X_ref bit for bit is returned
 * U_ref and X_ref bit for bit.  A row's outputs depend on neither B, its place in the batch, nor P; no atomics.
 * Stateless and asynchronous as gmpc_ensemble_rollout is (two launches at most, the same workspace rule).  Every
 * refusal is GMPC_EINVAL with a message starting "ensemble feedback: ", before any launch: gmpc_ensemble_rollout's
 * list (x0 excepted), a null X_ref, U_ref or K, exactly one of u_lo / u_hi, a non-finite alpha. */
int gmpc_ensemble_rollout_feedback(gmpc_ctx* ctx, int B, int S, int P, const float* dyn_members, const float* x0,
                                   const float* X_ref, const float* U_ref, const float* K, const float* k, float alpha,
                                   const float* u_lo, const float* u_hi, const float* goal, float* X, float* U,
                                   float* costs, float* obj, float* x_mean, float* x_var, void* stream);

/* A penalty on the members' one-step disagreement with the nominal model along a sampled row: a
 * property of the context, like the precision, the ensemble and its mode; off until set.  No stream, no device work.
 * Independent of the ensemble and of gmpc_set_params: neither resets it, it may be set before an ensemble is, and it
 * has no effect while none is set.  With GMPC_DIS_ONESTEP and an ensemble set, every launch over sampled rows rolls
 * the rows out under the context's bound (nominal) dynamics, once per member p, and plane p's cost is
 *   J_p = J + penalty * D_p,   D_p = sum_{t<T} sum_{j<n} (o^p_{t,j} - o^0_{t,j})^2,
 * J the row's cost of a solve without an ensemble, o^0_t = MLP_0([x_t; u_t]) the nominal network's output (bias
 * included, before the residual add) at the nominal rollout's x_t, o^p_t member p's output on the same input; D_p in
 * fp32, t ascending; the product rounded to fp32 before it is added.  The planes go through the aggregate of
 * gmpc_set_sampled_ensemble_mode with Q = P.  A member equal to the nominal layers has D_p == 0 exactly.  penalty may
 * have either sign (negative: exploration) and may be 0.  A non-finite member makes its own plane's cost NaN.
 * `samples`, X and obj are as under gmpc_set_sampled_ensemble.  In bf16 mode both passes run on the bf16 operands;
 * the difference, the sums and J stay fp32.
 * GMPC_EINVAL ("disagreement: ...", the setting left as it was) for a null ctx, a kind outside 0..1, a non-finite
 * penalty, penalty != 0 with GMPC_DIS_OFF, and a context the sampling solvers refuse.  While it is on and an ensemble is
 * set, a solve under a mode with GMPC_ENS_TS1 is refused before any launch ("disagreement: not with TS1 propagation").
 * gmpc_mppi_vjp stays refused while an ensemble is set. */
enum { GMPC_DIS_OFF = 0, GMPC_DIS_ONESTEP = 1 };
int gmpc_set_sampled_disagreement(gmpc_ctx* ctx, int kind, float penalty);

/* The one-step disagreement of every member with the bound dynamics along a plan: the forward-
 * only, stateless sibling of gmpc_ensemble_rollout for the quantity above.  dyn_members, x0, U, B, S, P as there.
 *   -> X [B][S+1][n]  the rollout under the bound (nominal) dynamics, X[b][0] = x0[b]
 *      d [P][B][S]    d_{p,t} = sum_j (o^p_{t,j} - o^0_{t,j})^2
 *      D [P][B]       the fp32 sum of d[p][b][:], t ascending
 *   each output may be NULL, not all of them.
 * fp32 whatever the sampled precision; the arithmetic of a row is that of the sampling solvers under
 * gmpc_set_sampled_disagreement, and a row's values depend on neither B, its place in the batch, nor P.  A non-finite
 * member makes its own planes non-finite and leaves the others' as they are.  Asynchronous on `stream` (one launch),
 * deterministic.  Every refusal is GMPC_EINVAL with a message starting "ensemble disagreement: ", before any launch: a
 * null ctx, dyn_members, x0 or U; B, S or P out of range; parameters not set; every output NULL; LSTM dynamics, a width
 * or n + m above 256. */
int gmpc_ensemble_disagreement(gmpc_ctx* ctx, int B, int S, int P, const float* dyn_members, const float* x0,
                               const float* U, float* X, float* d, float* D, void* stream);

/* The vector-Jacobian product of gmpc_ensemble_disagreement's d and D; the whole horizon only
 * (S = T).
 *   dyn_members [P][dyn_param_count], 1 <= P <= 16, 1 <= B <= max_batch as there, passed per call (nothing is kept)
 *   X [B][T+1][n]: the nominal rollout for U [B][T][m], as gmpc_ensemble_disagreement returns it
 *   gd [P][B][T] = dL/dd, gD [P][B] = dL/dD: either may be NULL, not both.  The weight of a step is
 *   w[p][b][t] = gd + gD (one fp32 addition; with one given, that value).
 * With z_t = [x_t; u_t], e^p_t = o^p_t - o^0_t and c^p_t = 2 w[p][b][t] e^p_t:
 *   q^p_t = (dMLP_p/dz)^T c^p_t;   c^N_t = -(((c^0_t + c^1_t) + ...) + c^{P-1}_t);   q^N_t = (dMLP_0/dz)^T c^N_t
 *   r_t = ((((q^0_t + q^1_t) + ...) + q^{P-1}_t) + q^N_t) = [rx_t; ru_t]
 *   lambda_T = 0, lambda_t = rx_t + lambda_{t+1} + (dMLP_0/dx)^T lambda_{t+1}   (through x_{t+1} = x_t + MLP_0(z_t))
 *   -> grad_x0 [B][n] = lambda_0;  grad_U [B][T][m], grad_U_t = ru_t + (dMLP_0/du)^T lambda_{t+1}
 *      grad_nominal [dyn_param_count] = sum_{b,t} (dMLP_0/dtheta)^T (c^N_t + lambda_{t+1}), w.r.t. the bound dynamics,
 *      in gmpc_set_params' dyn layout (the two deltas are added per row and layer, then summed over the rows)
 *      grad_members [P][dyn_param_count], row p = sum_{b,t} (dMLP_p/dtheta)^T c^p_t
 *   each output may be NULL (its work is skipped), not all of them.
 * The relu masks are recomputed from (X, U) under each network's layers (a unit is active iff its output is > 0).  Goals,
 * costs, mpc_w and the cost MLP do not enter.  fp32 whatever the sampled precision; deterministic (no atomics, fixed
 * orders): a problem's gradients depend on neither B nor its place in the batch, grad_members[p] neither on P nor on
 * the other members' cotangents.  A member whose layers equal the bound layers has e = 0 exactly: its row of
 * grad_members and its q^p are exact zeros.  A non-finite member makes its own row of grad_members and the shared
 * outputs non-finite and leaves the other rows as they are.
 * Stateless like gmpc_ensemble_rollout_vjp: the bound dynamics are read; a set sampled ensemble, its mode, the
 * disagreement setting, the sampled precision and a held solution are neither read nor changed.  Asynchronous on
 * `stream`, except that the first call needing more call workspace than the ctx holds allocates it (a synchronising
 * hipMalloc) and keeps it, in floats: P dyn_param_count + (P+1) B T (2 n + m) + B (T+1) n + 2 B T m, (P+1) B T (dyn
 * hidden layers) 8 mask words, and with grad_members or grad_nominal (2 P + 3) (B T + 8) (summed dyn widths).
 * Every refusal is GMPC_EINVAL with a message starting "ensemble disagreement vjp: ", before any launch: a null ctx,
 * dyn_members, X or U; B or P out of range; parameters not set; both cotangents NULL; every output NULL; LSTM
 * dynamics, a width or n + m above 256. */
int gmpc_ensemble_disagreement_vjp(gmpc_ctx* ctx, int B, int P, const float* dyn_members,
                                   const float* X, const float* U,
                                   const float* gd, const float* gD,
                                   float* grad_x0, float* grad_U,
                                   float* grad_nominal, float* grad_members, void* stream);

/* The vector-Jacobian product of gmpc_ensemble_rollout's X and costs under every member: per
 * member p the derivation of gmpc_rollout_vjp with f_p(x, u) = x + MLP_p([x; u]), taken at (X[p], U, goal) as passed,
 * under that member's cotangents; the whole horizon only (S = T).
 *   dyn_members [P][dyn_param_count] as for gmpc_ensemble_rollout, passed per call (nothing is kept); 1 <= P <= 16
 *   X [P][B][T+1][n]: member p's states for U [B][T][m], as gmpc_ensemble_rollout returns them; goal [B][T+1][n];
 *   1 <= B <= max_batch
 *   gX [P][B][T+1][n] = dL/dX, gcost [P][B][T+1] = dL/dcosts: either may be NULL, not both
 *   -> grad_x0 [B][n], grad_U [B][T][m], grad_goal [B][T+1][n] (row T is 0): ((g^0 + g^1) + ...) + g^{P-1} of the
 *      members' gradients, one fp32 addition per member in ascending p starting from member 0's value, so with P = 1
 *      the member's value comes through bit for bit
 *      grad_theta_sum [3 + cost_count] in gmpc_rollout_vjp's layout, SUMMED over the batch and the members in a fixed
 *      order; all zeros (as is grad_goal) when gcost is NULL
 *      grad_members [P][dyn_param_count], each row in gmpc_set_params' dyn layout, SUMMED over the batch, one row per
 *      member
 *   each output may be NULL (its work is skipped), not all of them.
 * The relu masks are recomputed from (X[p], U) under member p's layers (a unit is active iff its output is > 0, as in
 * gmpc_rollout_vjp).  fp32 whatever the sampled precision; deterministic (no atomics, fixed orders): a problem's
 * gradients depend on neither B nor its place in the batch, grad_members[p] not on P.  A non-finite member makes its
 * own row of grad_members and the shared sums non-finite and leaves the other rows as they are.
 * Stateless like gmpc_ensemble_rollout: mpc_w and the cost MLP of the bound parameters are read; a set sampled
 * ensemble, its mode, the disagreement setting, the sampled precision and a held solution are neither read nor
 * changed.  Asynchronous on `stream`, except that the first call needing more call workspace than the ctx holds
 * allocates it (a synchronising hipMalloc) and keeps it, in floats: P dyn_param_count (the members' transposes)
 * + P B n (with grad_x0) + P B T m (with grad_U) + P B (T+1) n (with grad_goal and gcost) + P B T (dyn hidden layers) 8
 * mask words; with gcost 2 (P B + 8) (summed cost widths), and with grad_theta_sum 3 P B + 8; with grad_members
 * 2 P (B T + 8) (summed dyn widths).
 * Every refusal is GMPC_EINVAL with a message starting "ensemble rollout vjp: ", before any launch: a null ctx,
 * dyn_members, X, U or goal; B or P out of range; parameters not set; both cotangents NULL; every output NULL; LSTM
 * dynamics, a width or n + m above 256. */
int gmpc_ensemble_rollout_vjp(gmpc_ctx* ctx, int B, int P, const float* dyn_members,
                              const float* X, const float* U, const float* goal,
                              const float* gX, const float* gcost,
                              float* grad_x0, float* grad_U, float* grad_goal,
                              float* grad_theta_sum, float* grad_members, void* stream);

/* a8-a11 (+a13/a16): upper-level loss and its bilevel gradient at the iLQR solution held by the ctx
 * after gmpc_ilqr_solve (policy/optimizers.py:61-73,78-105), per trajectory; the batch mean of
 * policy/base.py:126-127 is left to the caller (it is where the multi-GPU all-reduce goes).
 *   loss_kind 0: L2 (norm/l2_policy.py:12-18), desired [B][T+1][n]
 *   loss_kind 1: JS generator (gan/js_policy.py:60-68) with critic params `critic`
 *   sign: +1 reproduces the reference as written, -1 the implicit-function gradient.
 *   -> loss [B]; grad_sum [3 + cost_count]: SUM over the batch of d/d(mpc_w, cost params). */
int gmpc_bilevel_grad(gmpc_ctx* ctx, int B, int loss_kind, const float* desired,
                      const float* critic, float sign, float* loss, float* grad_sum, void* stream);

/* a8-a11 for a caller-defined upper-level loss, at the iLQR solution held by the ctx (the reference's `loss` is any
 * callable, policy/optimizers.py:34-83, policy/base.py:84-85): the caller passes lx = dL/dX [B][T+1][n] (xc columns;
 * carry columns included for LSTM dynamics) and/or lu = dL/dU [B][T][m] (either may be NULL, not both); then
 * Bvec_t = lu_t + B_t^T mu_{t+1}.  -> grad_sum [3 + cost_count], the SUM over the batch, as gmpc_bilevel_grad.
 * Follows gmpc_ilqr_solve, gmpc_ilqr_solve_fused or gmpc_ilqr_solve_box_held of the same B (else GMPC_EINVAL, "must precede"); leaves the
 * same ctx state as gmpc_bilevel_grad (Bvec, H, dX: debug buffers 4 / 2 / 3).  lx and lu are only read; with
 * lx NULL the ctx's own lx buffer (debug buffer 11) is zeroed and used.  With lu NULL and the lx that
 * gmpc_bilevel_grad computes, the result is bit-identical to gmpc_bilevel_grad's. */
int gmpc_bilevel_grad_cotangent(gmpc_ctx* ctx, int B, const float* lx, const float* lu, float sign,
                                float* grad_sum, void* stream);

/* The gradients of the same upper-level loss with respect to the solver's inputs, through the held solution:
 * grad_x0 [B][n] = dL/dx0 (xc: carry columns included for LSTM dynamics) and grad_goal [B][T+1][x_size] = dL/dgoal
 * (row T is 0: the terminal cost does not read it).  The TRUE derivative: no reference-compatibility sign.
 * Must follow gmpc_bilevel_grad or gmpc_bilevel_grad_cotangent of the same B on the same held solution (else
 * GMPC_EINVAL, "... must precede"): it reads the H and dX (and, for LSTM dynamics, the curvature) those leave.  Any
 * solve, gmpc_upper_loss or other call that drops the held solution voids them.
 * lx = dL/dX [B][T+1][n] as passed to the bilevel call; NULL means the ctx's own lx buffer -- the one
 * gmpc_bilevel_grad filled (L2 / JS), or the zeroed one gmpc_bilevel_grad_cotangent used for a NULL lx.  A caller
 * who passed their own lx passes it again.  Either output may be NULL, not both.  A non-NULL grad_x0 on the
 * step-major pipeline (n > 64 or m > 32: [A_t | B_t] is not kept) fails with GMPC_EINVAL; grad_goal works there.
 * Read-only for every existing ctx buffer (Bvec, H, dX, grad_sum stay as they were). */
int gmpc_bilevel_grad_inputs(gmpc_ctx* ctx, int B, const float* lx, float* grad_x0, float* grad_goal, void* stream);

/* The gradient of the same upper-level loss with respect to the dynamics network's weights, through the held
 * solution: grad_dyn_sum [dyn param count] in gmpc_set_params' dyn layout (per layer W_l, then b_l), summed over the
 * batch.  The TRUE derivative: no reference-compatibility sign.  Same precondition and lx as
 * gmpc_bilevel_grad_inputs (it reads the H and dX the bilevel call left, and [A_t | B_t], QT, qT of the solution).
 * Relu-MLP dynamics only: LSTM dynamics (dyn_lstm_features > 0) and the step-major pipeline (n > 64 or m > 32)
 * fail with GMPC_EINVAL, as do a NULL output and a missing bilevel call; nothing is launched then.
 * Read-only for every existing ctx buffer, in either order with gmpc_bilevel_grad_inputs; deterministic (fixed
 * reduction order, no atomics).  Workspace: about 2 B T (sum of the dyn widths) floats twice, allocated by the first
 * call that needs more than the ctx holds (a synchronising allocation) and kept for later calls. */
int gmpc_bilevel_grad_dynamics(gmpc_ctx* ctx, int B, const float* lx, float* grad_dyn_sum, void* stream);

/* The vector-Jacobian product of the rollout and its per-step costs (gmpc_rollout_cost's X and costs; trajax
 * rollout / evaluate at policy/optimizers.py:24-31) for a caller's cotangents gX = dL/dX [B][T+1][n] and
 * gcost = dL/dcosts [B][T+1] (either may be NULL, not both), taken at (X, U, goal) as passed: X must be the rollout
 * of (X[:, 0], U) under the bound parameters.  The TRUE derivative (no bilevel step, no reference sign):
 *   grad_x0 [B][n], grad_U [B][T][m], grad_goal [B][T+1][n] (row T is 0: the terminal cost does not read it) per
 *   trajectory; grad_theta_sum [3 + cost_count] in gmpc_bilevel_grad's grad_sum layout (mpc_w, then the cost MLP)
 *   and grad_dyn_sum [dyn param count] in gmpc_set_params' dyn layout, both SUMMED over the batch.
 * Any output may be NULL (its work is skipped: no weight-gradient rows without grad_dyn_sum), not all of them.
 * One reverse sweep through each step's relu MLP (the masks recomputed from (X, U) into the call's own workspace);
 * no [A_t | B_t] is formed, so every shape the ctx accepts is covered, the step-major ones (n > 64 or m > 32)
 * included.  Relu-MLP dynamics only: LSTM dynamics (dyn_lstm_features > 0), gX and gcost both NULL, every output
 * NULL, a NULL X / U / goal, B outside [1, max_batch] or no gmpc_set_params fail with GMPC_EINVAL before any launch.
 * Stateless and read-only for every existing ctx buffer: drops no held solution (see the ordering contract).
 * Deterministic (fixed reduction order, no atomics); asynchronous, except that the first call needing more workspace
 * than the ctx holds allocates it (a synchronising hipMalloc) and keeps it: B T (dyn hidden layers) 8 mask words,
 * with grad_theta_sum 2 (B + 8) (summed cost widths) + 3 B floats, with grad_dyn_sum 2 (B T + 8) (summed dyn
 * widths) floats. */
int gmpc_rollout_vjp(gmpc_ctx* ctx, int B, const float* X, const float* U, const float* goal,
                     const float* gX, const float* gcost,
                     float* grad_x0, float* grad_U, float* grad_goal,
                     float* grad_theta_sum, float* grad_dyn_sum, void* stream);

/* a13/a16 only: the upper-level loss [B] at the solution held by the ctx, without the gradient
 * (test-loss evaluation, norm/cost_trainer.py:13-21). */
int gmpc_upper_loss(gmpc_ctx* ctx, int B, int loss_kind, const float* desired, const float* critic,
                    float* loss, void* stream);

/* a19: Polyak blend out = factor*prev + (1-factor)*cur over a flat range (norm/cost_trainer.py:88-92).
 * out may alias prev or cur. */
int gmpc_polyak(gmpc_ctx* ctx, long count, const float* prev, const float* cur, double factor,
                float* out, void* stream);

/* a14-a15: critic BCE loss and gradient (gan/js_policy.py:41-58, critic/nn.py:28-42).
 *   xseq [Bc][T+1][n], label [Bc] (+1 / -1), critic params
 *   -> loss_sum [1] (SUM over the batch of -log p), grad_sum [critic_count] (SUM over the batch). */
int gmpc_critic_loss_grad(gmpc_ctx* ctx, int Bc, const float* xseq, const float* label,
                          const float* critic, float* loss_sum, float* grad_sum, void* stream);

/* a14/a16: critic scores and (optionally) d score / d xseq.
 *   -> score [Bc]; dxseq [Bc][T+1][n] or NULL. */
int gmpc_critic_score_vjp(gmpc_ctx* ctx, int Bc, const float* xseq, const float* critic,
                          float* score, float* dxseq, void* stream);

/* The vector-Jacobian product of the critic's scores at (critic, xseq) for a caller's output delta
 * g_score = dL/dscore [Bc]: any discriminator or generator objective is a function of the scores, and everything
 * behind the head's scalar output is linear in g_score.
 *   xseq [Bc][T+1][x_size], critic the flat parameters (layout above), g_score [Bc]
 *   -> score [Bc]; grad_xseq [Bc][T+1][x_size] = g_b * d score_b / d xseq_b per sequence; grad_critic_sum
 *      [critic_count] = sum_b g_b * d score_b / d theta in gmpc_critic_loss_grad's layout, SUMMED over the batch and
 *      overwritten.  Any output may be NULL (its work is skipped: no weight-gradient accumulation or GEMMs without
 *      grad_critic_sum, no dx without grad_xseq), but not both gradients.
 * The true derivative: no reference sign applies.  g = 1 gives gmpc_critic_score_vjp's dxseq, g = the BCE delta
 * gmpc_critic_loss_grad's grad_sum, g = -1 the generator cotangent of gmpc_bilevel_grad(loss_kind = 1).
 * One forward sweep, one head pass and one backward pass on every dispatch route of the critic step (register-weight
 * n <= 32 at F = 64, run-time n at F = 64, any other F <= 128, wide input n + F > 256); with both gradients the
 * register-weight backward sweep accumulates the LSTM weight gradient and writes dx in the same pass.
 * A NULL xseq, critic or g_score, both gradient outputs NULL, Bc outside [1, 2 max_batch] or a ctx created without a
 * critic fail with GMPC_EINVAL before any launch.
 * Stateless: it writes the critic step's own workspace and the caller's outputs only -- none of Bvec, H, dX or the
 * ctx's lx -- and drops neither a held solution nor a bilevel tail (see the ordering contract), so it may run between
 * a solve, its bilevel call and the inputs / dynamics calls.  Deterministic (fixed reduction order, no atomics):
 * identical calls give identical bits.  Asynchronous; no allocation. */
int gmpc_critic_vjp(gmpc_ctx* ctx, int Bc, const float* xseq, const float* critic, const float* g_score,
                    float* score, float* grad_xseq, float* grad_critic_sum, void* stream);

/* The second-order VJP of the critic's scores: what a gradient penalty (WGAN-GP, R1) differentiates.  With
 * g_b = d score_b / d xseq_b, any penalty P = sum_b p(g_b) has dP/dtheta = sum_b v_b . d g_b / d theta at v_b = dp/dg_b
 * held constant, and v_b . g_b is the directional derivative sdot_b = <d score_b / d xseq_b, v_b>: the output of the
 * tangent (forward-mode) critic run beside the primal one.  This call is the forward of (score, sdot) and one reverse
 * sweep for a caller's delta g_dir = dL/dsdot [Bc]; no Hessian is formed.
 *   xseq, v_xseq [Bc][T+1][x_size], critic the flat parameters (layout above), g_dir [Bc]
 *   -> score [Bc] (may be NULL); sdot [Bc]; grad_xseq [Bc][T+1][x_size] = g_b * d sdot_b / d xseq_b per sequence;
 *      grad_critic_sum [critic_count] = sum_b g_b * d sdot_b / d theta in gmpc_critic_loss_grad's layout,
 *      SUMMED over the batch and overwritten; its head-bias ranges are written as zeros (the biases reach sdot
 *      through the relu masks only, which are piecewise constant).  Either gradient may be NULL (its work is skipped);
 *      with both NULL the call is the forward only and g_dir may be NULL too.
 * Shapes: every critic with x_size + lstm_features <= 256 (one run-time-shape form, expf / tanhf activations, its own
 * saves and its own [Wx; Wh] transpose: on the register-weight shapes `score` agrees with gmpc_critic_score_vjp to
 * parity, not bit for bit).  The wide-input route (x_size + lstm_features > 256) fails with GMPC_EINVAL,
 * "unsupported shape".  A NULL xseq, critic, v_xseq or sdot, a gradient output without g_dir, Bc outside [1, 2 max_batch] or a ctx
 * created without a critic fail with GMPC_EINVAL before any launch.
 * Stateless, deterministic (fixed reduction order, no atomics) and asynchronous as gmpc_critic_vjp: it drops neither a
 * held solution nor a bilevel tail.  Per-call memory comes from the context's call workspace, which grows to the
 * largest call seen (gmpc_create allocates nothing for it). */
int gmpc_critic_dir_vjp(gmpc_ctx* ctx, int Bc, const float* xseq, const float* critic, const float* v_xseq,
                        const float* g_dir, float* score, float* sdot, float* grad_xseq, float* grad_critic_sum,
                        void* stream);

/* a18: optax.chain(clip_by_global_norm(max_norm), adam(lr)) on one contiguous trainable range
 * (gan/runner.py:51-63).  grad is scaled by grad_scale first (1/B for a batch sum).
 * step = 1-based update count.  params, m, v [count] are updated in place.  The hyper-parameters
 * are doubles: 1-b1, 1-b2 and the bias corrections are formed in double and rounded once to fp32,
 * as optax does with its Python-float hyper-parameters. */
int gmpc_adam_clip_step(gmpc_ctx* ctx, long count, float* params, const float* grad, float* m,
                        float* v, float grad_scale, int step, double lr, double max_norm, double b1,
                        double b2, double eps, void* stream);

/* e: the ONE exchange of an optimiser step -- the batch mean at policy/base.py:126-127 (cost /
 * generator step) and gan/js_policy.py:55 (critic step) -- for callers without torch.distributed: an
 * in-place SUM over ranks of the packed fp32 buffer [loss_sum | grad_sum | sample count] with RCCL over
 * xGMI (ncclAllReduce, ncclFloat32, ncclSum), enqueued on `stream`; the caller then divides by the
 * reduced count (or folds 1/count into gmpc_adam_clip_step's grad_scale).  One process per GPU:
 * rank 0 calls gmpc_comm_unique_id and hands the 128 bytes to the other ranks by its own means (file,
 * socket, MPI), every rank calls gmpc_comm_init(ctx, world_size, rank, id) -- collective -- once.
 * A ctx without gmpc_comm_init is a world of one and gmpc_allreduce_grads is a no-op.  RCCL is bound
 * at run time (dlopen): inside a PyTorch process the copy torch loaded is used.  The Python package
 * uses torch.distributed (backend "nccl" = the same RCCL) for this exchange, gan_mpc_amd/parallel.py. */
int gmpc_comm_unique_id(char* id128);
int gmpc_comm_init(gmpc_ctx* ctx, int world_size, int rank, const char* id128);
int gmpc_comm_world(gmpc_ctx* ctx, int* world_size, int* rank);
int gmpc_allreduce_grads(gmpc_ctx* ctx, float* packed, long count, void* stream);

/* N2: the expert sequence model that produces goal_xseq / init_useq for every solve
 * (policy/eval.py:87-107 get_goal_states_init_actions; expert/expert_model.py:60-91;
 * expert/nn.py:10-61).  lstm_features > 0: LSTMCell variant (x -> LSTM(F) -> y), == 0: StackedMLPCell
 * variant (y = relu(Dense(x)), head_dims[0] = that hidden width).  Both heads are relu MLPs
 * y -> ... -> n (state, residual: next_x = head + x) and y -> ... -> m (action, tanh).
 * Flat parameter layout `expert` (flax order, kernel (in,out) then bias):
 *   LSTM: Wx[n][4F] | Wh[F][4F] | b[4F] (gates i,f,g,o)   or   MLP: W0[n][h] | b0[h]
 *   then the state head's layers, then the action head's layers.
 * history [B][hist+1][n] (hist >= 1 teacher-forced rows, then the current state) ->
 * goal [B][T+1][x_size] (row 0 = current state), init_U [B][T][m].  x_size, m and the head widths up to 1024
 * (the C4 / C5 state sizes), F <= 128, the MLP variant's first width <= 512. */
typedef struct gmpc_expert_shape {
  int lstm_features;
  int head_layers;                           /* dense layers per head (>= 1) */
  int head_dims_x[GMPC_MAX_LAYERS + 1];      /* y width, hidden..., n */
  int head_dims_u[GMPC_MAX_LAYERS + 1];      /* y width, hidden..., m */
} gmpc_expert_shape;
int gmpc_expert_rollout(gmpc_ctx* ctx, int B, int hist, const gmpc_expert_shape* es,
                        const float* expert, const float* history, float* goal, float* init_U,
                        void* stream);
long gmpc_expert_param_count(int n, const gmpc_expert_shape* es);

/* Training of the expert sequence model: expert/trainer.py:10-31 (calculate_loss under jax.value_and_grad,
 * :34-58) with expert/nn.py:10-61 and utils.py:231-240 (discounted_sum).  For each of the B windows, from the
 * zero carry: x_in_t = teacher_forcing ? xseq[t] : next_x_{t-1} (x_in_0 = xseq[0]), (next_x_t, u_t) = model(x_in_t),
 * loss = sum_t discount^t (|u_t - useq[t]|^2 + |next_x_t - next_xseq[t]|^2), the discount built by repeated
 * fp32 multiplication.  The LSTM carry is fed back in both modes.
 *   xseq, next_xseq [B][S][x_size], useq [B][S][m], expert in the layout of gmpc_expert_rollout
 *   -> loss_sum [1], grad_sum [gmpc_expert_param_count] in the same flat layout: SUMS over the batch,
 *      overwritten (the caller divides by the global batch).  grad_sum == NULL: the loss only.
 * S >= 1 is independent of the ctx's T; B <= max_batch; caps as gmpc_expert_rollout (F <= 128, x_size, m and
 * head widths <= 1024, the MLP variant's first width <= 512); anything else fails with GMPC_EINVAL before any
 * launch.  Workspace: the ctx keeps buffers for the BPTT rows (B * S of them) and grows them on the first call
 * that needs more (hipMalloc / hipFree: that call allocates and synchronises); every later call of the same or
 * a smaller size only enqueues work.  Fixed reduction order, no atomics: identical calls give identical bits. */
int gmpc_expert_loss_grad(gmpc_ctx* ctx, int B, int S, const gmpc_expert_shape* es, const float* expert,
                          const float* xseq, const float* useq, const float* next_xseq, double discount,
                          int teacher_forcing, float* loss_sum, float* grad_sum, void* stream);

/* The vector-Jacobian product of gmpc_expert_rollout at (expert, history) for a caller's cotangents
 * g_goal = dL/dgoal [B][T+1][x_size] and g_U = dL/dinit_U [B][T][m] (either may be NULL, not both; a NULL one is zero):
 *   grad_expert_sum [gmpc_expert_param_count] in the flat layout of gmpc_expert_rollout, SUMMED over the batch and
 *   overwritten; grad_history [B][hist+1][x_size] per window.  Either output may be NULL (its work is skipped: no
 *   weight-gradient rows or GEMMs without grad_expert_sum), not both.
 * The schedule is the rollout's: steps st = 0 .. hist+T-1, the input of step st is history[st] for st <= hist and the
 * previous step's next_x after that, goal[st-hist+1] = next_x_st and init_U[st-hist] = u_st for st >= hist,
 * goal[0] = history[hist].  So g_goal[:, 0] goes straight into grad_history[:, hist]; the teacher-forced steps
 * st < hist receive gradient through the LSTM carry only, and for the MLP variant (no carry) rows < hist of
 * grad_history are exactly zero.  The action head is differentiated through its tanh.  T is the ctx's horizon.
 * Caps as gmpc_expert_rollout (F <= 128, x_size, m and head widths <= 1024, the MLP variant's first width <= 512),
 * hist >= 1, 1 <= B <= max_batch; anything else, both cotangents NULL or both outputs NULL fail with GMPC_EINVAL
 * before any launch.  Stateless and read-only for every existing ctx buffer: drops no held solution and no bilevel
 * tail (see the ordering contract), so it may run between a solve, its bilevel call and the inputs / dynamics calls.
 * Deterministic (fixed reduction order, no atomics); asynchronous, except that the first call needing more workspace
 * than the ctx holds allocates it (a synchronising hipMalloc) and keeps it: up to 2 (B (hist+T) + 8) row strides
 * (gmpc_expert_loss_grad's rows), B (hist+T) (6F + m) save floats and one transposed copy of the weights. */
int gmpc_expert_vjp(gmpc_ctx* ctx, int B, int hist, const gmpc_expert_shape* es, const float* expert,
                    const float* history, const float* g_goal, const float* g_U,
                    float* grad_expert_sum, float* grad_history, void* stream);

/* N3: dynamics-model regression, norm/dynamics_trainer.py:14-47 (predict_loss) and
 * :62-86 (batch mean + value_and_grad) with utils.py:230-240 (discounted_sum).  For each of the B
 * sequences: x_in_t = teacher_forcing ? xseq[t] : pred_{t-1} (x_in_0 = xseq[0]),
 * pred_t = dynamics(x_in_t, useq[t]), loss = sum_t discount^t |pred_t - next_xseq[t]|^2.
 *   xseq, next_xseq [B][S][n], useq [B][S][m], 1 <= S <= T, B <= max_batch
 *   -> loss_sum [1] (sum over the batch), grad_sum [dynamics parameter count] in the flat flax
 *      order of gmpc_set_params' dyn vector (sum over the batch: divide by the global batch size).
 * Uses the dynamics parameters bound by gmpc_set_params (n + m up to 1088: C4 / C5 included).  LSTM variant:
 * x columns only (xseq, next_xseq [B][S][x_size]), the carry starts at zero and is fed back even under teacher
 * forcing (dynamics_trainer.py:24-33); grad_sum in the layout Wx | Wh | b | tail. */
int gmpc_dynamics_loss_grad(gmpc_ctx* ctx, int B, int S, const float* xseq, const float* useq,
                            const float* next_xseq, double discount, int teacher_forcing,
                            float* loss_sum, float* grad_sum, void* stream);

/* The same regression for the P members of a dynamics ensemble in one call, on the matrix cores (DESIGN.md section
 * 25): member p's weights are dyn_members + p * (dynamics parameter count), each laid out like gmpc_set_params' dyn.
 *   xseq, next_xseq [D][S][n], useq [D][S][m]: the dataset, D >= 1 rows; 1 <= S <= T
 *   rows [P][B] (int32, each in [0, D): trusted, the host binding checks them): the dataset row that member p uses as
 *        its b-th sequence -- duplicates allowed, so a dataset is uploaded once and every member draws its own
 *        bootstrap minibatch; NULL: D == B and the identity for every member
 *   -> loss_sum [P], grad_sum [P][dynamics parameter count]: sums over member p's B sequences, 1 <= B <= max_batch
 * Relu-MLP dynamics with every width and n + m up to 256 (what gmpc_sampled_coverage accepts), 1 <= P <= 16.  Reads
 * nothing of the dynamics bound by gmpc_set_params (which need not have been called) and leaves a held solution, the
 * bilevel tail and a set sampled ensemble untouched.  Asynchronous on `stream`; deterministic.  Every refusal is
 * GMPC_EINVAL with a message starting "ensemble fit: ", before any launch.  Workspace: the call workspace, grown (a
 * synchronising hipMalloc) by the first call that needs more: 2 P (B S + 8) row strides, P parameter counts for the
 * transposed weights and P B losses. */
int gmpc_dynamics_ensemble_loss_grad(gmpc_ctx* ctx, int P, const float* dyn_members, int D, int B, int S,
                                     const float* xseq, const float* useq, const float* next_xseq, const int* rows,
                                     double discount, int teacher_forcing, float* loss_sum, float* grad_sum,
                                     void* stream);

/* Building block of the large-state (n > 64) Riccati path, exported for its unit test: batched
 * C[b] = alpha * X[b]^T Y[b] + beta * C[b] on the fp32 matrix cores; X[b] is K x M, Y[b] K x N,
 * C[b] M x N, row-major, densely packed per batch element; Y must be followed by >= 8 readable rows
 * of N floats (N < 64: by max(8 N, 4 N + 256) floats, see gmpc_bgemm_desc). */
int gmpc_bgemm_tn(gmpc_ctx* ctx, int batch, int M, int N, int K, const float* X, const float* Y,
                  float* C, float alpha, float beta, void* stream);

/* The same family with every argument the large-state pass sets, for the unit tests (tests/bgemm_cases.py):
 *   C[b] = alpha * (X[b]^T Y[b] + X2[b]^T Y2[b] + X3[b]^T Y3[b]) + beta * C[b] + E[b][:, 0:En],
 * then the rows of C[b] whose bit in rowmask[b] is clear (bit r & 31 of word r >> 5, srm words per batch element) are
 * set to 0.  X*[b] is K* x M, Y*[b] K* x N with leading dimensions ld* >= the width and batch strides s* (in floats;
 * 0 shares an operand); K2 = 0 / K3 = 0, E = NULL, rowmask = NULL switch a part off.  Batch elements whose `active`
 * entry is 0 are left untouched (active = NULL: all of them).  upper_only (M = N, a symmetric result): entries below
 * the diagonal may be left unwritten.  Y[b] + K * ldy must be followed by max(8 * ldy, 4 * ldy + 256) readable floats. */
typedef struct gmpc_bgemm_desc {
  int batch, M, N, K;
  const float* X; long sx; int ldx;
  const float* Y; long sy; int ldy;
  float* C; long sc; int ldc;
  float alpha, beta;
  const int* active;
  const float* X2; long sx2; int ldx2;
  const float* Y2; long sy2; int ldy2;
  int K2;
  const float* X3; long sx3; int ldx3;
  const float* Y3; long sy3; int ldy3;
  int K3;
  int upper_only;
  const float* E; long se; int lde; int En;
  const unsigned* rowmask; long srm;
} gmpc_bgemm_desc;
int gmpc_bgemm_tn_ex(gmpc_ctx* ctx, const gmpc_bgemm_desc* d, void* stream);
/* The kernel form gmpc_bgemm_tn_ex launches for `d`, without GPU work (the pointers are only compared with NULL):
 * route4 = {0, NTW, 0, 0} one-wave strips k_bgemm_tn<NTW>; {1, WIDE_X, NTJ, NS} streaming k_bthin;
 * {2, WNT, KC, VEC} LDS-staged k_bgemm_tn_lds<2, WNT, KC, VEC>. */
int gmpc_bgemm_route(const gmpc_bgemm_desc* d, int* route4);

/* The weight-gradient GEMM behind every weight and bias gradient, for the unit tests (tests/wgrad_cases.py):
 *   C[M][N] = sum_{r < rows} A[r][0:M]^T B[r][0:N],   colsum[N] = sum_{r < cs_rows} B[r][0:N]   (colsum = NULL: none)
 * with leading dimensions lda >= M, ldb >= N and 1 <= cs_rows <= rows.  `part` is the caller's buffer of part_floats
 * floats for the partial sums: its content afterwards is unspecified, nothing is written behind it.  mfma_ok allows the
 * matrix-core kernels and promises GMPC_WGRAD_PAD = 8 allocated, finite rows behind row rows - 1 of B, and of A as well
 * when N == 1 && M % 32 == 0; no other float outside the logical matrices is used.  form = GMPC_WGRAD_AUTO: the
 * launcher every gradient call uses; GMPC_WGRAD_COLSUM_ONLY: the column sums alone (over `rows` rows; A, C, M, lda and
 * cs_rows are ignored).  In a batch, a problem with M == 0 and C == colsum is its column sums alone (over cs_rows). */
enum { GMPC_WGRAD_AUTO = 0, GMPC_WGRAD_COLSUM_ONLY = 1 };
typedef struct gmpc_wgrad_desc {
  int rows, M, N, lda, ldb, cs_rows;
  const float* A; const float* B;
  float* C; float* colsum;
  int mfma_ok, form;
  float* part; long part_floats;
} gmpc_wgrad_desc;
/* One problem.  GMPC_EINVAL (before any GPU call) for a bad argument, colsum with cs_rows < 1 among them, and for a
 * column-sum-only call whose `part` holds fewer than N floats. */
int gmpc_wgrad_ex(gmpc_ctx* ctx, const gmpc_wgrad_desc* d, void* stream);
/* np problems through the batch kernel with one partial-sum buffer (the problems' own part / part_floats / mfma_ok /
 * form are ignored).  *taken = 0: the batch does not qualify (np > 8, a problem with N % 128 != 0, rows < 64,
 * ldb % 4 != 0 or B not 16-byte aligned, a buffer too small); nothing was launched and nothing written. */
int gmpc_wgrad_batch_ex(gmpc_ctx* ctx, const gmpc_wgrad_desc* probs, int np, float* part, long part_floats,
                        void* stream, int* taken);
/* The launcher's decision for `d` without GPU work (the pointers are compared with NULL, never followed):
 * route6 = {form, NTW, rows per chunk, chunks, rows per column-sum chunk, column-sum chunks}; form 0 = the VALU kernel
 * k_wgrad (NTW = 0; chunks = its row splits), 1 = k_wgrad_mfma<NTW>, 2 = k_wgrad_mfma<NTW> on swapped operands
 * (N == 1), 3 = column sums alone.  The last two are 0 where no separate column-sum kernel runs. */
int gmpc_wgrad_route(const gmpc_wgrad_desc* d, int* route6);
/* Whether gmpc_wgrad_batch_ex would take the batch: route2 = {taken, rows per chunk} (B is tested for alignment). */
int gmpc_wgrad_batch_route(const gmpc_wgrad_desc* probs, int np, long part_floats, int* route2);

/* The dynamics Jacobian chain on its own, for the unit tests (tests/linearize_cases.py):
 *   AB[s] = [A | B] = W_L^T D_{L-1}(s) W_{L-1}^T ... D_1(s) W_1^T + [I | 0],   s = 0 .. nsamp - 1,   AB [nsamp][n][n+m]
 * with the weights (and their padded copies) of the ctx's last gmpc_set_params, through the dispatch of the backward
 * passes.  D_l(s) comes from the caller's relu bits: masks holds 8 words per (sample, hidden layer), the words of
 * sample s and hidden layer l (0-based) at [((s * samp_mul + samp_add) * Lh + l) * 8], unit u in bit u & 31 of word
 * u >> 5; all 8 words are read, and bits at or past the layer's width may be set (they select zero pad rows).
 * `active` (NULL: every sample) is read at (s * samp_mul + samp_add) / T: a sample whose entry is 0 is either left
 * untouched or written with its Jacobian.  GMPC_EINVAL for a NULL ctx / masks / AB, nsamp < 1, samp_mul < 1,
 * samp_add < 0, before gmpc_set_params, and for a ctx with LSTM dynamics or the low-rank large-state form. */
int gmpc_linearize_ex(gmpc_ctx* ctx, int nsamp, const unsigned* masks, const int* active, float* AB, int samp_mul,
                      int samp_add, void* stream);
/* The chain gmpc_linearize_ex and the backward passes launch for a ctx of `shape` and nsamp samples (strided != 0: any
 * samp_mul / samp_add but 1 / 0), without GPU work.  route[0] = family: 0 none, 1 k_linearize_sparse,
 * 2 k_linearize_regs, 3 k_linearize_mfma, 4 the VALU k_linearize, 5 LSTM dynamics, 6 low-rank factors.  For MLP
 * dynamics the rest is the plan of k_linearize_mfma<NT, NTF> for the launch, whichever family takes it: route[1..3] =
 * NT, NTF, NGF (column tiles of the hidden GEMMs, of one group of the input GEMM, groups), route[4] / route[5] = the
 * padded W_1^T / W_L staged in LDS, route[6] = input-GEMM body (0 fed from the seed: one hidden layer; 1 the six-deep
 * ring: NTF = 1; 2 multi-tile), route[7] = 32-row tiles, route[8] = workgroups, route[9] = LDS bytes of one,
 * route[10] = mask rows of a tile's slab, route[11] = 1 when k_linearize_mfma accepts the launch. */
#define GMPC_LIN_ROUTE_INTS 12
int gmpc_linearize_route(const gmpc_shape* shape, int nsamp, int strided, int* route);

/* Number of candidate rollouts (trajectory, step size) the line searches of the last gmpc_ilqr_solve
 * evaluated -- the work count behind bench.py's secondary roofline.  Synchronises the whole device
 * (hipDeviceSynchronize). */
long gmpc_linesearch_candidates(gmpc_ctx* ctx);

/* Counters of the line searches of the last gmpc_ilqr_solve, `n` <= 64 values: out[k], k = 0..15 = line searches
 * that accepted the step alpha_0 / 2^k (trajax line_search_ddp as called from policy/optimizers.py:19), out[16] =
 * line searches that ran out of step sizes, out[17] = the deepest halving accepted since the solve began, out[24 + r] =
 * candidate rollouts of speculative round r.  Diagnostic (bench.py reports it); synchronises the whole device
 * (hipDeviceSynchronize: streams created non-blocking included). */
int gmpc_linesearch_stats(gmpc_ctx* ctx, long* out, int n);

/* Stream overlap hook.  `hip_event` (a hipEvent_t, or NULL to clear) is recorded on the backward pass's stream
 * behind the Jacobian chain of gmpc_lqr_backward(_after_rollout) / of every iteration of gmpc_ilqr_solve.  Order of
 * the small-state pass: terminal quadratisation, Jacobian chain, EVENT, Riccati sweep (the terminal quadratisation
 * needs X only and runs first, so that the sweep is the launch right behind the chain).  Large-state path: the event
 * is recorded at the top of the pass, before the terminal quadratisation and the step-major pipeline.  A caller that
 * runs independent work on a second stream -- the critic step of the GAN loop: reference gan/runner.py:120-168 has no
 * data dependence between it and the policy's backward pass -- makes that stream wait for the event: the work then
 * shares the chip with the Riccati sweep (two wavefronts per trajectory: most wave slots and registers are free)
 * instead of taking workgroup slots from the matrix-core-bound Jacobian chain.  The event must outlive its use. */
int gmpc_set_linearize_event(gmpc_ctx* ctx, void* hip_event);

/* Optional per-kernel timing with HIP events recorded on the launch stream around each kernel
 * (bench.py's roofline leg).  Slots: 0 rollout, 1 linearize, 2 terminal, 3 riccati, 4 linesearch,
 * 5 lstm_fwd, 6 head, 7 lstm_bwd, 8 wgrad (all weight-gradient GEMMs of one critic call), 9 adam.
 * gmpc_profile_read waits for the recorded events, returns the summed milliseconds and the number
 * of launches of that slot since the last read, and resets the slot. */
int gmpc_profile_enable(gmpc_ctx* ctx, int on);
int gmpc_profile_read(gmpc_ctx* ctx, int slot, double* total_ms, int* count);
/* Name of the kernel the slot's last launch ran on, as it appears in a rocprofv3 kernel trace (slot 1, the
 * Jacobian chain: the instantiation the shape selected, e.g. "k_linearize_regs<6, 100, 8, false>"); "" for slots
 * that always run the same kernel.  The string lives in the context (copied when the chain is launched): valid until
 * the context's next backward pass or gmpc_destroy. */
const char* gmpc_profile_kernel_name(gmpc_ctx* ctx, int slot);

/* Device pointers into the ctx's solution of the last gmpc_ilqr_solve / gmpc_bilevel_grad (valid
 * until the next such call): 0 X, 1 U, 2 H = A^-1 B, 3 dX, 4 Bvec, 5 AB, 6 K, 7 k, 11 d loss / d X.
 * Buffer 5 holds [B][T][n][n+m] for n <= 64 and ONE step's [B][n][n+m] (the last one processed,
 * t = 0) for n > 64.  gmpc_debug_buffer_count returns the number of floats allocated behind the
 * pointer (for max_batch trajectories); a reader must not go past it.
 * Used by the parity tests and by EvalMPC.get_optimal_values' `lqr` slot. */
const float* gmpc_debug_buffer(gmpc_ctx* ctx, int which);
long gmpc_debug_buffer_count(gmpc_ctx* ctx, int which);

#ifdef __cplusplus
}
#endif
#endif
