// Every host function that is defined in one .hip file and called from another, by defining file; that file includes
// this header too, so each definition is checked against what its callers see.  Default arguments live here only.
// (gmpc_fused_solve.h keeps the one-launch solves' argument blocks and limits beside their prototypes.)
#pragma once
#include "gmpc_device.h"     // (and with it the device helpers: a kernel file needs this include only)

// gmpc_api.hip: the thread's error record behind gmpc_last_error(); returns `code`
int gmpc_fail(int code, const char* fmt, ...);

// gmpc_traj.hip ------------------------------------------------------------------------------------------------------
void gmpc_launch_rollout(const TrajArgs& a, hipStream_t s);
// the general trajectory kernel: one workgroup per 4 trajectories (ls = false) / work-list items (ls = true)
void gmpc_launch_traj(const TrajArgs& a, bool ls, int grid, hipStream_t s);
// masks: [B][T][Lh][GMPC_MW] relu bits of the dynamics' hidden layers at (X_t, U_t)
void gmpc_launch_masks(int B, int n, int m, int T, const MlpDesc& dyn, const float* X, const float* U,
                       uint32_t* masks, hipStream_t s);
// gmpc_traj_rw.hip: the register-weight trajectory kernel
bool gmpc_traj_rw_shape(const TrajArgs& a);
// LDS of one workgroup; sets the sizing fields of `a`
size_t gmpc_traj_rw_lds(TrajArgs& a);
void gmpc_launch_traj_rw(const TrajArgs& a, bool ls, int grid, size_t lds, hipStream_t s);
// gmpc_ls16.hip / gmpc_ls32.hip: 16 / 32 line-search candidates per workgroup; the shapes they are instantiated for
bool gmpc_ls16_shape(const TrajArgs& a);
bool gmpc_ls32_shape(const TrajArgs& a);
// one workgroup per 16 / 32 work-list items; `max_items` bounds the list (the kernel reads the actual count)
void gmpc_launch_ls16(const TrajArgs& a, long max_items, hipStream_t s);
void gmpc_launch_ls32(const TrajArgs& a, long max_items, hipStream_t s);

// gmpc_linesearch.hip -------------------------------------------------------------------------------------------------
// step sizes alpha_0 / 2^k, k = 0, 1, .., that stay above alpha_min (trajax' loop), counted up to `cap`
int gmpc_ls_halvings(float alpha_0, float alpha_min, int cap);
// The route of a solve's line searches: everything about them that its shape, options and the GMPC_LS* variables fix.
struct LsPlan {
  bool rw, ls16, ls32;      // kernels that evaluate candidates beside a custom evaluator's / k_traj<true>: k_traj_rw<true>,
                            // and with it k_ls16, and with that k_ls32
  int split16, split32;     // TrajArgs::ls_split / ls32_split (0: form not taking part; else 1 <= split16 <= split32)
  int k_max;                // gmpc_ls_halvings
  int first_min;            // least size of a trajectory's first round
  int rounds;               // rounds enqueued per line search (the worst case)
  int aw, pw, sw0, swl;     // k_traj_rw's LDS sizing (the TrajArgs fields) and bytes
  size_t lds;
};
// `a`: B, shape, networks, alpha_0 / alpha_min; ncu: compute units of the device; non-zero: more than
// GMPC_LS_ROUNDS_MAX rounds
int gmpc_ls_plan(const TrajArgs& a, int ncu, bool custom_eval, LsPlan* p);
// `eval` (optional, custom_eval of the plan): another evaluator of the candidates of a round -- the LSTM dynamics
// variant (gmpc_dynl.hip) -- behind the same work list and the same decide / commit kernels; `user` is handed back to it
typedef void (*gmpc_ls_eval_fn)(void* user, const TrajArgs&, int max_items, hipStream_t);
void gmpc_launch_linesearch(const TrajArgs& a, const LsPlan& p, const LsWork& w, hipStream_t s,
                            gmpc_ls_eval_fn eval = nullptr, void* user = nullptr);

// gmpc_backward.hip ---------------------------------------------------------------------------------------------------
// VALU Jacobian chain; non-zero when the row count of n is not instantiated
int gmpc_launch_linearize(int B, int T, int n, int m, const MlpDesc& dyn, const uint32_t* masks, const int* active,
                          float* AB, hipStream_t s);
// terminal quadratisation QT [B][n][n], qT [B][n]; non-zero on an unsupported cost fout
int gmpc_launch_terminal(int B, int T, int n, const MlpDesc& cm, const float* mpc_w, const float* X, const int* active,
                         float* QT, float* qT, hipStream_t s);
void gmpc_launch_riccati(const RiccatiArgs& a, hipStream_t s);
// gmpc_riccati_w.hip: the two-wave sweep
bool gmpc_riccati_w_shape(const RiccatiArgs& a);      // mode 0 only; GMPC_RICCATI=valu keeps k_riccati
bool gmpc_riccati_w2h_shape(const RiccatiArgs& a);    // mode 1 with the loss adjoint folded in (MLP dynamics)
// k_riccati_w2 in the mode of a.mode; lx, lu (optional), bvec_out: the Hessian solve's loss adjoint, mode 1 only
void gmpc_launch_riccati_w(const RiccatiArgs& a, const float* lx, const float* lu, float* bvec_out, hipStream_t s);

// Jacobian chains (gmpc_linearize_*.hip) -----------------------------------------------------------------------------
// All of them: Jacobians of NSamp samples; sample s is sample s*samp_mul + samp_add of `masks`.  They return 0 on
// launch and -1 when the shape is not one the form covers (the caller takes the next form).
int gmpc_launch_linearize_sparse(int NSamp, int T, int n, int m, const MlpDesc& dyn, const LinPad& lp,
                                 const uint32_t* masks, const int* active, float* AB, int samp_mul, int samp_add,
                                 hipStream_t s);
int gmpc_launch_linearize_regs(int NSamp, int T, int n, int m, const MlpDesc& dyn, const LinPad& lp,
                               const uint32_t* masks, const int* active, float* AB, int samp_mul, int samp_add,
                               hipStream_t s);
// rows row0..n-1 of every sample (row0 = 0: all of them; the wide form takes row0 = 0 only)
int gmpc_launch_linearize_regs_rows(int NSamp, int T, int n, int m, const MlpDesc& dyn, const LinPad& lp,
                                    const uint32_t* masks, const int* active, float* AB, int samp_mul, int samp_add,
                                    int row0, hipStream_t s);
const char* gmpc_linearize_regs_last_name();   // instantiation the last gmpc_launch_linearize_regs* launched
int gmpc_launch_linearize_mfma(int NSamp, int T, int n, int m, const MlpDesc& dyn, const LinPad& lp,
                               const uint32_t* masks, const int* active, float* AB, int samp_mul, int samp_add,
                               hipStream_t s);
// The mask contract of every chain.  masks holds GMPC_MW words per (sample, hidden layer), at
// [((s * samp_mul + samp_add) * Lh + l) * GMPC_MW + word]; bit u & 31 of word u >> 5 is the relu bit of unit u of hidden
// layer l (0-based; its width is dims[l + 1]).  Bits at or past a layer's width MAY be set.  k_linearize_mfma reads
// all GMPC_MW words of every (sample, layer) of the launch and only meets such bits in k-steps whose weight rows are
// the zero pad rows of both operands (odd widths, the read-ahead), so they select zeros; k_linearize_regs (widths 64,
// 128, 200) reads only the words its width spans; k_linearize_sparse (200-wide layers) reads words 0..6 and clips
// word 6 to its 8 units, so it never sees them.  (tests/linearize_cases.py sets such bits for k_linearize_mfma.)  `active` (null: everything) is read at
// (s * samp_mul + samp_add) / T; a sample whose entry is 0 is either left untouched or written with its Jacobian (a
// 32-row tile is skipped only when every sample it touches is inactive).
//
// The decisions of the chains apart from their launches (host only; gmpc_linearize_route exports them for
// tests/linearize_cases.py).  Column tiles of the padded operands: NT of the hidden GEMMs, NTF per group of the input
// GEMM, NGF groups.
void gmpc_linpad_tiles(int L, const int* dims, int n, int m, int* NT, int* NTF, int* NGF);
enum { LIN_BODY_SINGLE = 0, LIN_BODY_RING = 1, LIN_BODY_MULTI = 2 };   // input GEMM: seed-fed / gemm_tile_1 / gemm_tile
struct LinMfmaPlan {
  int NT, NTF, NGF;
  int ntiles, nsmax;          // 32-row tiles; most samples a tile touches (the slab's mask rows)
  int stage_w1, stage_wl;     // the padded W_1^T / W_L are copied to LDS (W_1^T first, each when it still fits)
  int grid, body;
  size_t lds;                 // dynamic LDS of one workgroup, <= GMPC_LIN_LDS_MAX
};
#define GMPC_LIN_LDS_MAX (160 * 1024)
// non-zero: k_linearize_mfma does not take the launch (2^31 rows or more, or the slabs alone exceed the LDS)
int gmpc_linearize_mfma_plan(long NSamp, int n, int m, int L, const int* dims, LinMfmaPlan* p);
// whether gmpc_launch_linearize_sparse / _regs / the VALU chain take a launch (what their launchers test first)
bool gmpc_linearize_sparse_covers(long NSamp, int n, int m, int L, const int* dims, bool strided);
bool gmpc_linearize_regs_covers(long NSamp, int n, int m, int L, const int* dims, int row0);
bool gmpc_linearize_valu_covers(int n);
// The order of the chains, in one place for gmpc_api_solve.hip's backward pass, gmpc_large.hip's step and
// gmpc_linearize_ex: LSTM dynamics -> their own kernel; large state (big) with lowrank_h > 0 -> the low-rank factors;
// then sparse (small state, unless GMPC_LIN=dense, read per call), regs, mfma, VALU (small state, whole batch only).
enum { LIN_NONE = 0, LIN_SPARSE = 1, LIN_REGS = 2, LIN_MFMA = 3, LIN_VALU = 4, LIN_DYNL = 5, LIN_LOWRANK = 6 };
int gmpc_linearize_family_of(bool big, int lowrank_h, bool dynl, long NSamp, int n, int m, int L, const int* dims,
                             bool strided);
// launches the chain of `family` (sparse, regs, mfma or VALU); non-zero when it is none of them or its launcher
// declines.  The VALU chain takes whole batches only: NSamp = B * T, samp_mul = 1, samp_add = 0.
int gmpc_launch_linearize_family(int family, int NSamp, int T, int n, int m, const MlpDesc& dyn, const LinPad& lp,
                                 const uint32_t* masks, const int* active, float* AB, int samp_mul, int samp_add,
                                 hipStream_t s);
// last hidden width when the large-state pass takes the low-rank form of the Jacobians for `sh`, else 0 (gmpc_large.hip)
int gmpc_big_lowrank_h(const gmpc_shape* sh);
// padded weight copies of the chains: floats of the buffer, and the build on every gmpc_set_params
size_t gmpc_linpad_floats(const gmpc_shape* sh);
void gmpc_linpad_prepare(const MlpDesc& dyn, int n, int m, float* pad, size_t pad_floats, LinPad* out, hipStream_t s);
// k_linearize_sparse's packed copies inside that buffer: floats they add (0: shape not covered), build at `p` (zeroed)
size_t gmpc_linsparse_floats(int L, const int* dims, int n, int m);
void gmpc_linsparse_prepare(const MlpDesc& dyn, int n, int m, float* p, LinPad* out, hipStream_t s);

// gmpc_bgemm.hip: the batched "TN" GEMM family ----------------------------------------------------------------------
void gmpc_launch_bgemm_tn(const BgemmArgs& a, hipStream_t s);
// the kernel form the dispatcher picks: strips p = {NTW}, thin p = {WIDE_X, NTJ, NS}, lds p = {WNT, KC, VEC}
enum { BGEMM_STRIPS = 0, BGEMM_THIN = 1, BGEMM_LDS = 2 };
struct BgemmRoute { int family; int p[3]; };
BgemmRoute gmpc_bgemm_route_of(const BgemmArgs& a);

// gmpc_big_step.hip: k_big_step for the a.B trajectories of step a.t --------------------------------------------------
// non-zero (nothing launched) when the step's LDS does not fit one workgroup per CU
int gmpc_launch_big_step(const BigStepArgs& a, hipStream_t s);

// gmpc_large.hip: the step-major pipeline (n > 64 or m > 32) ---------------------------------------------------------
// one backward pass, non-zero when no Jacobian kernel covers the shape; lx / Bvec (lu optional): the bilevel tail's
int gmpc_big_backward(const BigWork& w, int B, const MlpDesc& dyn, const LinPad& lp, const uint32_t* masks,
                      const float* X, const float* U, const float* goal, const float* mpc_w, const float* QT,
                      const float* qT, const int* active, float* K, float* k, float* grad, float* adj, const float* lx,
                      float* Bvec, hipStream_t s, const DynlDesc* dl = nullptr, const float* lam_sol = nullptr,
                      const float* lu = nullptr);
// the bilevel tail's forward tangent roll; X / U: the solution, read by the LSTM variant (dl) only
int gmpc_big_forward_tangent(const BigWork& w, int B, const MlpDesc& dyn, const LinPad& lp, const uint32_t* masks,
                             const float* K, const float* k, float* Hout, float* dX, hipStream_t s,
                             const DynlDesc* dl = nullptr, const float* X = nullptr, const float* U = nullptr);
void gmpc_launch_big_cont(int B, int T, int m, const float* U, const float* gn2, const int* iters, const float* obj,
                          const float* alpha, const float* obj_step, const float* U_step, const gmpc_ilqr_opts& opts,
                          const int* active, int* cont, hipStream_t s);

// gmpc_critic.hip: the critic LSTM sweeps outside gmpc_critic_lstm.hip's shapes (F = 64 with n > 32 or on the wide-input
// path, where cd.n == 0 and xproj holds x_t Wx; any other F <= 128) ---------------------------------------------------
void gmpc_launch_lstm_fwd(int Bc, const CriticDesc& cd, const float* xseq, float* gates, float* cs, float* hp,
                          float* hT, const float* xproj, hipStream_t s);
void gmpc_launch_lstm_bwd(int Bc, const CriticDesc& cd, const float* gates, const float* cs, const float* dhT,
                          float* dz, float* dxseq, hipStream_t s);

// gmpc_optim.hip: optimiser and utility kernels ----------------------------------------------------------------------
void gmpc_launch_transpose(int R, int C, const float* in, float* out, hipStream_t s);   // in [R][C] -> out [C][R]
void gmpc_launch_transpose_all(const TransposeList& mats, hipStream_t s);   // a list of them in one launch
void gmpc_launch_mlp_transpose_all(const MlpDesc& d, hipStream_t s);        // every W[l] -> WT[l] in one launch
void gmpc_launch_sum(int count, const float* v, float* out, int square, hipStream_t s);
void gmpc_launch_adam(long count, float* p, const float* g, float* m, float* v, float scale, int step, double lr,
                      double max_norm, double b1, double b2, double eps, float* scratch /* >= 257 */, hipStream_t s);
void gmpc_launch_polyak(long count, const float* prev, const float* cur, double f, float* out, hipStream_t s);

// gmpc_wgrad.hip -----------------------------------------------------------------------------------------------------
// The weight-gradient GEMM: C[M][N] = sum_r A[r][:M]^T B[r][:N]; colsum[N] = sum_{r < cs_rows} B[r][:N] (optional; no
// rows, cs_rows < 1, give zeros).
// Its matrix-core kernel k_wgrad_mfma reads its streamed operand up to GMPC_WGRAD_PAD rows past `rows`; the other
// operand is clamped to its last row and masked to zero there, so those rows only have to be allocated and finite.  The
// streamed operand is B -- except on the transposed route (N == 1 and M % 32 == 0: C^T = sum_r B_r^T A_r), where it is
// A.  So mfma_ok promises GMPC_WGRAD_PAD pad rows behind B, and behind A as well whenever N == 1 && M % 32 == 0.  The
// batch kernel (k_wgrad_batch) and the VALU kernel (k_wgrad) read no row past `rows` of either operand.
#define GMPC_WGRAD_PAD 8
#define GMPC_WGRAD_MAX_SPLIT 256   // most row chunks of the VALU form (k_wgrad)
// The launcher's decision, apart from its launch (host only; gmpc_wgrad_route exports it for tests/wgrad_cases.py).
// rpc / nchunks: rows per chunk and chunks of the GEMM part (VALU: rows per split, splits); crpc / cchunks: those of the
// separate column-sum kernel (matrix-core forms and WGRAD_COLSUM; 0 without colsum).  direct: the VALU form with a
// buffer too small for one partial sum writes its single split straight to C / colsum and leaves `part` alone.
enum { WGRAD_VALU = 0, WGRAD_MFMA = 1, WGRAD_MFMA_SWAPPED = 2, WGRAD_COLSUM = 3 };
struct WgradRoute { int form, ntw, rpc, nchunks, crpc, cchunks; bool direct; };
WgradRoute gmpc_wgrad_route_of(int rows, int M, int N, bool colsum, int cs_rows, long part_floats, bool mfma_ok);
// part holds part_floats floats (<= 0: unbounded) and no form writes past them: up to GMPC_WGRAD_MAX_SPLIT partial sums
// of M*N + N floats, fewer where they would not fit; mfma_ok: the pad rows above are there
void gmpc_launch_wgrad(int rows, int M, int N, const float* A, int lda, const float* Bm, int ldb, float* C,
                       float* colsum, int cs_rows, float* part, hipStream_t s, long part_floats, bool mfma_ok);
// One MLP's rows summed into its packed gradient g = W_0 | b_0 | W_1 | b_1 | ... (the layout of a parameter vector):
// `acts` and `dels` are [rows + GMPC_WGRAD_PAD][r.stride] in the layout of `r` (MlpRows); the biases sum the first
// cs_rows rows.  Returns g behind the last layer.
float* gmpc_launch_wgrad_mlp(int rows, int cs_rows, int L, const int* dims, const float* acts, const float* dels,
                             const MlpRows& r, float* g, float* part, long part_floats, hipStream_t s);
// all problems in one launch (+ one reduction); false when one does not qualify (the caller issues them one by one).
// gmpc_wgrad_batch_plan is its decision without the launches: the common rows per chunk (0: the batch does not
// qualify) and every problem's tiling and slices of `part` (host only, B is only tested for alignment).
int gmpc_wgrad_batch_plan(WgProb* probs, int np, long part_floats);
bool gmpc_launch_wgrad_batch(WgProb* probs, int np, float* part, long part_floats, hipStream_t s);
// colsum[N] = sum_{r < rows} B[r][:N] on its own (two launches; `part` holds the chunk sums, at most part_floats of
// them); false, and nothing launched, when part_floats < N
bool gmpc_launch_colsum(int rows, int N, const float* Bm, int ldb, float* colsum, float* part, long part_floats,
                        hipStream_t s);

// gmpc_critic_lstm.hip: second-generation LSTM kernels (n <= 32) and the head ----------------------------------------
bool gmpc_lstm2_supported(const CriticDesc& cd);
long gmpc_lstm2_wpart_floats(const CriticDesc& cd, int Bc);   // floats of the weight-gradient partial buffer
bool gmpc_launch_lstm_fwd2(int Bc, const CriticDesc& cd, const float* xseq, float* G, float* Cst, float* Hst, float* hT,
                           hipStream_t s);
// Wp != null: weight gradients -> gWx, gWh, gb (sums over the Bc sequences); dxseq != null: input gradient
bool gmpc_launch_lstm_bwd2(int Bc, const CriticDesc& cd, const float* xseq, const float* G, const float* Cst,
                           const float* Hst, const float* dhT, float* Wp, float* gWx, float* gWh, float* gb,
                           float* dxseq, hipStream_t s);
#define GMPC_HEAD2_LD 264     // leading dimension of plast: 256 products + dscore, padded to a multiple of 8
void gmpc_launch_head2(int Bc, const CriticDesc& cd, int loss_kind, const float* hT, const float* label, float* score,
                       float* loss, float* acts, float* dels, float* plast, float* dhT, const MlpRows& rows,
                       hipStream_t s);

// gmpc_critic_dir.hip: the tangent critic and its reverse sweep (gmpc_critic_dir_vjp), n + F <= 256 ----------------------
bool gmpc_dir_supported(const CriticDesc& cd);
size_t gmpc_dir_save_floats(const CriticDesc& cd, int Bc);     // floats behind DirSaves (without A)
void gmpc_dir_bind_saves(const CriticDesc& cd, int Bc, float* save, DirSaves* sv);
// primal and tangent forward sweep of (xseq, vseq); fills sv (and sv.A where set)
void gmpc_launch_dir_fwd(int Bc, const CriticDesc& cd, const float* xseq, const float* vseq, const DirSaves& sv,
                         hipStream_t s);
// score (optional), sdot; with g_dir the reverse of the tangent head: sv.dhd and the acts / dels rows (layout `rows`,
// needs cd.head.WT)
void gmpc_launch_dir_head(int Bc, const CriticDesc& cd, const DirSaves& sv, const float* g_dir, float* score, float* sdot,
                          float* acts, float* dels, const MlpRows& rows, hipStream_t s);
// dual BPTT (needs cd.WcatT); D [2 R][4F] = [z~ ; zd~] and dxseq are optional
void gmpc_launch_dir_bwd(int Bc, const CriticDesc& cd, const DirSaves& sv, float* D, float* dxseq, hipStream_t s);

// gmpc_bilevel.hip ----------------------------------------------------------------------------------------------------
void gmpc_launch_l2loss(int B, int T, int n, int ng, const float* X, const float* desired, float* loss, float* lx,
                        hipStream_t s);
void gmpc_launch_bvec(int B, int T, int n, int m, const float* AB, const float* lx, const float* lu, float* Bvec,
                      hipStream_t s);
// the clamped set of a held box solve, [B][T] words (bit j: control j); u_lo / u_hi [m] or null; m <= 32
void gmpc_launch_box_clamped(int B, int T, int m, const float* U, const float* grad, const float* u_lo,
                             const float* u_hi, uint32_t* clamped, hipStream_t s);
void gmpc_launch_costvjp(int B, int T, int n, int m, const MlpDesc& cm, const float* mpc_w, float sign, const float* X,
                         const float* U, const float* goal, int ng, const float* Hc, const float* dX, float* gmpc,
                         float* cact, float* cdel, const MlpRows& rows, hipStream_t s);
void gmpc_launch_get_cost(int B, int n, int ng, int m, const MlpDesc& cm, const float* mpc_w, const float* x,
                          const float* u, const float* goal_row, int terminal, float* out, hipStream_t s);

// gmpc_tail_adjoints.hip ----------------------------------------------------------------------------------------------
// The adjoint sweeps over the held solution.  X, dX, lx [B][T+1][n], goal [B][T+1][ng], AB [B][T][n][n+m],
// QT [B][n][n], mpc_w [3].
struct TailAdjArgs {
  int B, T, n, ng, m;
  const float *mpc_w, *X, *goal, *dX, *lx, *AB, *QT;
  // the inputs call: H [B][T][m]; Phi [B][T][n+m][n+m] or null (relu dynamics); gx0 [B][n]; ggoal [B][T+1][ng] or null
  const float *H, *Phi;
  float *gx0, *ggoal;
  // the dynamics call: qT [B][n]; the planes w = mu_{t+1} - nu_{t+1} and lam_{t+1}, [B][T][n]
  const float* qT;
  float *w, *lam;
};
// planes false: the inputs call, true: the dynamics call; non-zero for n > 64 or m > 32 (no [A_t | B_t] is kept), or
// when one step with Phi exceeds the LDS budget
int gmpc_launch_tail_adjoints(const TailAdjArgs& a, bool planes, hipStream_t s);
void gmpc_launch_goal_grad(int B, int T, int n, int ng, const float* mpc_w, const float* X, const float* goal,
                           const float* dX, float* ggoal, hipStream_t s);

// gmpc_dyn_grads.hip --------------------------------------------------------------------------------------------------
// acts / dels: 2 B T rows in the layout `lay` of the dynamics MLP.  Widths up to 256; returns 1 otherwise.
int gmpc_launch_dyn_rows(int B, int T, int n, int m, const MlpDesc& dyn, const float* X, const float* U,
                         const float* dX, const float* H, const float* w, const float* lam, float* acts, float* dels,
                         const MlpRows& lay, hipStream_t s);

// The sampled rollout of the sampling solvers: k_sampled_rollout of gmpc_cem_rollout.h, instantiated over
// CEM's rows (gmpc_cem.hip; MPPI's too) and iCEM's pool (gmpc_icem.hip), each with fp32 or bf16 matrix operands (§23)
// and under one model or every member of a dynamics ensemble (§24).  What it covers -- here for the launcher and for
// the entry points' messages:
#define GMPC_SAMPLED_MAX_WIDTH 256   // every layer width of both MLPs, and n + m
#define GMPC_CEM_MAX_N 4096          // rows per problem (the sort's keys: 32 KiB of LDS)
// A dynamics ensemble: one grid row of workgroups per member, then k_ens_reduce.  The arguments' dyn describes member
// 0 (bf16: with W[l] at its packed images); member p's weights lie p wstride floats behind them, its biases p bstride
// floats; part [P][B][ldc] takes the members' costs and the arguments' costs [B][ldc] their sum in member order times
// 1 / P (the default mode).
// The ensemble mode (gmpc_set_sampled_ensemble_mode): Q cost planes instead of P -- Q = P with ts1 == 0,
// plane q member q as above; with ts1 the grid row q is a particle that draws its member anew at every step
// (CemParticle of gmpc_cem_rollout.h) and Q is the number of particles -- and `aggregate` (GMPC_ENS_MEAN / MEAN_STD /
// MAX) is the rule that takes part [Q][B][ldc] to costs; invQ = 1.0f / (float)Q, risk the multiple of the spread.
// The one-step disagreement (gmpc_set_sampled_disagreement): with `disagree` (never with ts1) the rows are
// rolled out under the nominal layers `nom` (bf16: W[l] at their packed images) and plane q's cost is the nominal cost
// plus penalty times member q's summed squared one-step deviation from them (CemDisagree of gmpc_cem_rollout.h).
#define GMPC_MAX_ENSEMBLE 16
struct CemNominal { const float *W[GMPC_MAX_LAYERS], *b[GMPC_MAX_LAYERS]; };
struct CemEnsemble {
  int P;
  size_t wstride, bstride;
  float* part;
  int Q, ts1, aggregate;
  float invQ, risk;
  int disagree;
  float penalty;
  CemNominal nom;
};

// gmpc_cem.hip: the cross-entropy method's two kernels --------------------------------------------------
// The noise stream of one iteration: Philox4x32-10 under the key (key0, key1), counter (element group, sample,
// problem, it); cbeta = sqrt(1 - beta^2) of the smoothing along time.
struct CemRng { uint32_t key0, key1, it; float beta, cbeta; };
// The rollout over CEM's rows: N sample rows per problem in tiles of 32; mean / sd [B][T][m]; lo / hi [m] or null.
// mean_row: the rows are the mean itself (std 0, no bounds; N = 1, and X [B][T+1][n] may be set).  costs [B][N];
// samples [B][N][T][m] or null.
struct CemRollArgs {
  int B, N, T, n, m, mean_row;
  MlpDesc dyn, cost;
  const float *mpc_w, *x0, *goal, *mean, *sd, *lo, *hi;
  CemRng rng;
  float *costs, *X, *samples;
};
// k_cem_update: the E smallest of costs [B][N] by (cost, index), mean / sd updated in place; elites [B][E] or null
struct CemUpdArgs {
  int B, N, E, T, m;
  const float *costs, *lo, *hi;
  float *mean, *sd;
  CemRng rng;
  float gamma;
  int* elites;
};
// Non-zero (nothing launched) outside the limits above.  bf16: dyn.W[l] / cost.W[l] point at the layers' packed bf16
// images (MlpDesc::W reinterpreted; gmpc_launch_pack_bf16).  ens: null, or the ensemble every member of which rolls the
// rows out, followed by the reduce into a.costs (two launches; no X).  mean_row: fp32 on one model only.
int gmpc_launch_sampled_rollout(const CemRollArgs& a, bool bf16, const CemEnsemble* ens, hipStream_t s);
int gmpc_launch_cem_update(const CemUpdArgs& a, hipStream_t s);
void gmpc_launch_ens_reduce(const CemEnsemble& e, int B, int rows, int ldc, float* costs, hipStream_t s);

// gmpc_ens_rollout.hip: a plan's rollout under every member of a dynamics ensemble -----------------------
// B problems in tiles of 32, one grid row of workgroups per member: x0 [B][n], U [B][S][m], 1 <= S <= T; dyn describes
// member 0 (fp32), member p lies p mstride floats behind it.  goal [B][T+1][n] or null: null skips the cost terms and
// the cost MLP; set, it needs S == T.  X [P][B][S+1][n], costs [P][B][T+1] (stage costs, the terminal cost at T) and
// obj [P][B] (their sum in step order) may each be null; costs and obj need goal.
struct EnsRollArgs {
  int B, S, T, n, m;
  MlpDesc dyn, cost;
  size_t mstride;
  const float *mpc_w, *x0, *U, *goal;
  float *X, *costs, *obj;
};
// Non-zero (nothing launched) outside the sampled rollout's coverage, 1 <= S <= T, 1 <= P <= GMPC_MAX_ENSEMBLE and the
// rules above
int gmpc_launch_ens_rollout(const EnsRollArgs& a, int P, hipStream_t s);
// The same rollout in closed loop: a.U is not read; per member and row u_t = clamp(U_ref[b][t] + K[b][t]
// (x_t - X_ref[b][t]) + alpha k[b][t], u_lo, u_hi).  X_ref [B][S+1][n], U_ref [B][S][m], K [B][S][m][n]; k [B][S][m]
// or null (no feed-forward term); u_lo / u_hi [m], both or neither (no clamp); U [P][B][S][m] the applied controls or
// null.  a.x0's rows lie x0_stride floats apart: n, or (S + 1) n when a.x0 is X_ref itself.
struct EnsFeedbackArgs {
  const float *X_ref, *U_ref, *K, *k, *u_lo, *u_hi;
  float alpha;
  size_t x0_stride;
  float* U;
};
// Non-zero (nothing launched) outside gmpc_launch_ens_rollout's rules and those above
int gmpc_launch_ens_rollout_feedback(const EnsRollArgs& a, const EnsFeedbackArgs& f, int P, hipStream_t s);
// A plan's one-step disagreement: the rows of gmpc_launch_ens_rollout rolled S steps under the nominal
// layers `nom` (fp32), member p (dyn: member 0, p mstride floats behind it) measured against them at every visited
// (x_t, u_t).  X [B][S+1][n] the nominal states, d [P][B][S] the squared deviations of the one-step outputs, D [P][B]
// their sums in step order; each may be null, not all of them.
struct EnsDisArgs {
  int B, S, n, m;
  MlpDesc dyn;
  size_t mstride;
  CemNominal nom;
  const float *x0, *U;
  float *X, *d, *D;
};
// Non-zero (nothing launched) outside the sampled rollout's coverage, S >= 1 and 1 <= P <= GMPC_MAX_ENSEMBLE
int gmpc_launch_ens_disagreement(const EnsDisArgs& a, int P, hipStream_t s);
// mean / var [count] (either may be null) over the planes X [P][count]: the sum in member order / P, the squared
// deviations' sum in member order / P
void gmpc_launch_ens_moments(const float* X, int P, size_t count, float* mean, float* var, hipStream_t s);

// gmpc_ens_rollout_vjp.hip: the VJP of that rollout and its costs under every member --------------------
// dyn describes member 0 -- W / b in the caller's [P][count] vectors, WT in the call's transposes, laid out alike --,
// member p lies p mstride floats behind it; cost: the bound cost MLP with its transposes.  X, gX [P][B][T+1][n], gc
// [P][B][T+1] (gX or gc may be null), U [B][T][m], goal [B][T+1][n].  masks: [P][B T][L-1][GMPC_MW] words of the call
// (unused for L == 1).  Per-member outputs, each may be null: gx0 [P][B][n], gU [P][B][T][m], ggoal [P][B][T+1][n]
// (written only with gc), gm [P B][3].  acts / dels: per member B T + GMPC_WGRAD_PAD rows in the layout dr, rstride
// floats apart, or both null; cacts / cdels: P B rows in the layout cr, needed with gc.
struct EnsVjpArgs {
  int B, T, n, m;
  MlpDesc dyn, cost;
  size_t mstride, rstride;
  MlpRows dr, cr;
  const float *mpc_w, *X, *U, *goal, *gX, *gc;
  uint32_t* masks;
  float *gx0, *gU, *ggoal, *gm;
  float *acts, *dels, *cacts, *cdels;
};
// The row pass (masks, acts) and the sweep: two launches.  Non-zero (nothing launched) outside the sampled rollout's
// coverage, 1 <= P <= GMPC_MAX_ENSEMBLE and the rules above.
int gmpc_launch_ens_rollout_vjp(const EnsVjpArgs& a, int P, hipStream_t s);
// out[s][i] = ((planes[s][0][i] + planes[s][1][i]) + ...) + planes[s][P-1][i], i < count[s], for up to three arrays in
// one launch (count 0: none)
struct EnsVjpReduce {
  int P;
  size_t count[3];
  const float* planes[3];
  float* out[3];
};
void gmpc_launch_ens_vjp_reduce(const EnsVjpReduce& r, hipStream_t s);

// gmpc_ens_disagree_vjp.hip: the VJP of a plan's one-step disagreement, its local part -------------------
// dyn describes member 0 as in EnsVjpArgs (W / b in the caller's [P][count] vectors, WT in the call's transposes, member
// p mstride floats behind it); nom: the bound dynamics with their transposes.  X [B][T+1][n] the nominal rollout, U
// [B][T][m]; gd [P][B][T] and gD [P][B], one may be null.  Planes of the call, plane P the nominal's: masks
// [P+1][B T][L-1][GMPC_MW] (unused for L == 1), out [P+1][B T][n] the networks' outputs, q [P+1][B T][n+m] the local
// input gradients.  rx [B][T+1][n] (row T zero) and ru [B][T][m]: their sum in ascending p, the nominal last.  acts /
// dels: per member B T + GMPC_WGRAD_PAD rows in the layout dr, rstride floats apart, or both null; ndels: the B T rows of
// the nominal's local deltas (c^N and what it becomes below the output layer), or null.
struct DisVjpArgs {
  int B, T, n, m, P;
  MlpDesc dyn, nom;
  size_t mstride, rstride;
  MlpRows dr;
  const float *X, *U, *gd, *gD;
  uint32_t* masks;
  float *out, *q, *rx, *ru;
  float *acts, *dels, *ndels;
};
// Three launches (k_disvjp_rows, k_disvjp_back, k_disvjp_reduce).  Non-zero (nothing launched) outside the sampled
// rollout's coverage, 1 <= P <= GMPC_MAX_ENSEMBLE and the rules above.
int gmpc_launch_dis_vjp_local(const DisVjpArgs& a, hipStream_t s);
// out[r][j] = x[r][j] + y[r][j] for j < width of `rows` rows ld floats apart; out may be x or y
void gmpc_launch_dis_vjp_add(size_t rows, int width, size_t ld, const float* x, const float* y, float* out,
                             hipStream_t s);

// gmpc_icem.hip: the sample-efficient cross-entropy method's two kernels --------------------------------
// The rows of one iteration's pool, per problem: rows 0 .. Nit-1 fresh samples (sample index = row), rows Nit ..
// Nit+carry-1 the first `carry` rows of keep [B][nkeep][T][m], then -- with addmean -- the mean itself; every row
// clamped to the bounds.  white: the fresh rows are cem_control's (no colouring); otherwise cw [T/2 + 1] are the
// weights of the coloured sum (gmpc_icem_plan_host).
struct IcemPool {
  int Nit, carry, addmean, nkeep, white;
  const float *keep, *cw;
};
// The rollout over the pool's rows; c.N is the stride of `samples` (fresh rows only), costs [B][ldc].
struct IcemRollArgs {
  CemRollArgs c;
  IcemPool p;
  int ldc;
  int zlds;      // set by the launcher: the T normals of every (row, control) of a tile are formed once, in LDS behind
                 // the operand blocks (where 32 m T floats fit there)
};
// k_icem_update: the E smallest of the pool's costs by (cost, row); mean / sd refit in place (left alone where no cost
// is finite); keep_out [B][nkeep][T][m] <- the controls of ranks 0 .. nkeep-1; best_cost [B] / best_U [B][T][m]
// (both or neither) take rank 0 where it is strictly cheaper; with `last`, U_out [B][T][m] (may be null) <- best_U
// where return_best and the best cost is finite, the new mean otherwise.  elites [B][E] pool rows, or null.
struct IcemUpdArgs {
  int B, E, T, m, ldc;
  IcemPool p;
  const float *costs, *lo, *hi;
  float *mean, *sd;
  CemRng rng;
  float gamma;
  int* elites;
  float *keep_out, *best_U, *best_cost, *U_out;
  int return_best, last;
  int stage;     // set by the launcher: elites per staged block of controls (0: one element per thread)
};
// CEM's limits with Nit + carry + addmean rows, bf16 and ens as there: non-zero (nothing launched) otherwise
int gmpc_launch_sampled_rollout(const IcemRollArgs& a, bool bf16, const CemEnsemble* ens, hipStream_t s);
int gmpc_launch_icem_update(const IcemUpdArgs& a, hipStream_t s);

// gmpc_sampled_bf16.hip: bf16 elements of the packed images of an MLP's layers (each a multiple of 8), and the pack
// of the fp32 weights src.W[l] into the images img.W[l] (one launch for both MLPs)
size_t gmpc_bf16_image_elems(int L, const int* dims);
void gmpc_bind_bf16_images(MlpDesc& img, const MlpDesc& src, void* base);
void gmpc_launch_pack_bf16(const MlpDesc& dyn, const MlpDesc& dyn_img, const MlpDesc& cost, const MlpDesc& cost_img,
                           hipStream_t s);

// gmpc_mppi.hip: the path-integral update on the costs of CEM's rollout, and its adjoint ----------------
// k_mppi_update: w_s = exp(-(costs_s - min) / lam) over the finite costs [B][N], mean <- gamma mean + (1 - gamma)
// sum_s w_s u_s / sum_s w_s in place; sd is read only.  weights [B][N] (normalised), mean_trace [B][T][m] (the mean
// before the update) and costs_copy [B][N] may be null.
struct MppiUpdArgs {
  int B, N, T, m;
  const float *costs, *lo, *hi, *sd;
  float* mean;
  CemRng rng;
  float gamma, lam;
  float *weights, *mean_trace, *costs_copy;
  int stage;     // set by the launcher: samples per staged block of products (0: one element per thread)
};
// k_mppi_cotangent: problems b0 .. b0 + Bc - 1, row r = (b - b0) N + s of the chunk workspace.  mean / sd / g
// [B][T][m], costs [B][N], x0 [B][n], goal [B][T+1][n] are indexed by b; Us [R][T][m], gc [R][T+1], x0r [R][n],
// goalr [R][T+1][n], wn [R] (the normalised weights) and nm [Bc][T][m] (new_mean) by the chunk's rows.
struct MppiCotArgs {
  int b0, Bc, N, T, n, m;
  const float *mean, *sd, *costs, *lo, *hi, *g, *x0, *goal;
  CemRng rng;
  float gamma, lam;
  float *Us, *gc, *x0r, *goalr, *wn, *nm;
};
// k_mppi_reduce: g [B][T][m] <- gamma g + sum_s [lo < u_s < hi] ((1 - gamma) wn_s g + GU_s); gx0 [B][n] and ggoal
// [B][T+1][n] (each may be null) += the sums of the rows Gx0 / Ggoal; all in sample order
struct MppiRedArgs {
  int b0, Bc, N, T, n, m;
  const float *lo, *hi, *wn, *Us, *GU, *Gx0, *Ggoal;
  float gamma;
  float *g, *gx0, *ggoal;
};
// N <= 4096 and lam > 0: non-zero (nothing launched) otherwise
int gmpc_launch_mppi_update(const MppiUpdArgs& a, hipStream_t s);
int gmpc_launch_mppi_cotangent(const MppiCotArgs& a, hipStream_t s);
void gmpc_launch_mppi_reduce(const MppiRedArgs& a, hipStream_t s);
void gmpc_launch_mppi_add(long count, const float* v, float* out, hipStream_t s);                // out[i] += v[i]
void gmpc_launch_mppi_bcast(int rows, int cols, const float* v, float* out, hipStream_t s);     // out[r][c] = v[r]

// gmpc_rollout_vjp.hip ------------------------------------------------------------------------------------------------
// masks: [B][T][Lh][GMPC_MW] relu bits at (X_t, U_t).  Null outputs are skipped; cacts / cdels (B rows in the cost
// MLP's layout cr) and gm go together; dels: B T rows in the dynamics MLP's layout dr.
void gmpc_launch_rvjp_sweep(int B, int n, int m, int T, const MlpDesc& dyn, const MlpDesc& cost, const float* mpc_w,
                            const float* X, const float* U, const float* goal, const float* gX, const float* gc,
                            const uint32_t* masks, float* gx0, float* gU, float* ggoal, float* gm, float* cacts,
                            float* cdels, float* dels, const MlpRows& dr, const MlpRows& cr, hipStream_t s);
// acts: B T rows in the layout dr (the layer inputs); masks as k_masks writes them
void gmpc_launch_rvjp_acts(int B, int n, int m, int T, const MlpDesc& dyn, const float* X, const float* U, float* acts,
                           const MlpRows& dr, uint32_t* masks, hipStream_t s);

// gmpc_dynfit.hip: dynamics regression --------------------------------------------------------------------------------
int gmpc_launch_dynfit(int B, int S, int n, int m, const MlpDesc& dyn, const float* xseq, const float* useq,
                       const float* yseq, float gamma, int teacher_forcing, float* pred, float* acts, float* dels,
                       const MlpRows& rows, float* loss, hipStream_t s);

// gmpc_dynfit_rows.hip: the same regression for the P members of an ensemble, on the matrix cores ---------
// dyn describes member 0 -- W / b in the caller's [P][count] vectors, WT in the call's transposes, laid out alike --,
// member p lies p mstride floats behind it.  xseq / yseq [D][S][n], useq [D][S][m]; rows [P][B] names the dataset row of
// each member's b-th sequence (null: D = B, the identity).  acts / dels: per member B S + GMPC_WGRAD_PAD rows in the
// layout `lay`, rstride floats apart; loss [P][B].
struct DynFitRowsArgs {
  int B, S, n, m;
  MlpDesc dyn;
  size_t mstride, rstride;
  MlpRows lay;
  const float *xseq, *useq, *yseq;
  const int* rows;
  float gamma;
  int teacher_forcing;
  float *acts, *dels, *loss;
};
// The transposes of every member into WT0 (= a.dyn.WT[0]), the sweeps and loss_sum [P]: three launches.  Non-zero, and
// nothing launched, outside widths and n + m <= GMPC_SAMPLED_MAX_WIDTH, 1 <= P <= GMPC_MAX_ENSEMBLE, or where the S
// discounts do not fit the workgroup's LDS.
int gmpc_launch_dynfit_rows(const DynFitRowsArgs& a, int P, float* WT0, float* loss_sum, hipStream_t s);
// its first launch alone: W_l -> W_l^T of every layer of the P members of `dyn` (as above) into WT0 (= dyn.WT[0])
void gmpc_launch_dynfit_transpose(const MlpDesc& dyn, size_t mstride, int P, float* WT0, hipStream_t s);

// gmpc_dynl.hip: LSTM dynamics variant --------------------------------------------------------------------------------
void gmpc_launch_dynl_rollout(DynlTrajArgs a, hipStream_t s);
void gmpc_launch_dynl_candidates(DynlTrajArgs a, int max_items, hipStream_t s);
// [A_t | B_t] / the curvature term Phi_t = lam_{t+1} . d^2 f of steps t0 .. t0 + nt - 1 of a T-step horizon
void gmpc_launch_dynl_jac(int B, int T, int nt, int t0, const DynlDesc& d, const float* X, const float* U,
                          const int* active, float* AB, hipStream_t s);
void gmpc_launch_dynl_curv(int B, int T, int nt, int t0, const DynlDesc& d, const float* X, const float* U,
                           const float* adj, const int* active, float* Phi, hipStream_t s);
void gmpc_launch_add_phi(int B, int n, int m, const float* Phi, float* HG, float* T1, hipStream_t s);
// the first nx of n columns of every row: src [rows][n] -> dst [rows][nx], and back (zero on the other columns)
void gmpc_launch_cols_gather(long rows, int n, int nx, const float* src, float* dst, hipStream_t s);
void gmpc_launch_cols_scatter(long rows, int n, int nx, const float* src, float* dst, hipStream_t s);
size_t gmpc_dynl_fit_stride(const DynlDesc& d);   // floats per acts / dels row: the LSTM columns, then the tail's
// tail: the tail MLP's MlpRows, its stride set to gmpc_dynl_fit_stride
void gmpc_launch_dynl_fit(int B, int S, const DynlDesc& d, const float* xseq, const float* useq, const float* yseq,
                          float gamma, int teacher_forcing, float* pred, float* acts, float* dels, const MlpRows& tail,
                          float* save, float* loss, hipStream_t s);

// gmpc_expert.hip / gmpc_expert_fit.hip -------------------------------------------------------------------------------
int gmpc_launch_expert(const ExpertArgs& a, hipStream_t s);   // non-zero on an unsupported shape
void gmpc_launch_expert_fit(const ExpertFitArgs& a, hipStream_t s);

// gmpc_expert_vjp.hip: floats of the save rows of one call; the transposes of a.net and the sweep (non-zero on an
// unsupported shape, before any launch)
size_t gmpc_expert_vjp_save_floats(const ExpertVjpArgs& a);
int gmpc_launch_expert_vjp(const ExpertVjpArgs& a, hipStream_t s);

// gmpc_comm.hip: multi-GPU exchange -----------------------------------------------------------------------------------
struct GmpcComm { void* comm = nullptr; int world = 1, rank = 0; };   // comm: the ncclComm_t, null in a world of one
int gmpc_comm_unique_id_impl(char* id128);
int gmpc_comm_init_impl(GmpcComm* gc, int world, int rank, const char* id128);
int gmpc_comm_allreduce_impl(GmpcComm* gc, float* packed, long count, hipStream_t s);
void gmpc_comm_destroy_impl(GmpcComm* gc);
