// Argument block and limits of the one-launch iLQR solves (gmpc_fused_solve.hip: gmpc_ilqr_solve_fused and its
// control-limited form gmpc_ilqr_solve_box).
#pragma once
#include "gmpc_device.h"

#define GMPC_FZ_NC 8          // line-search candidates evaluated together (the rows of one forward pass)
#define GMPC_FZ_JR 16         // rows of one pass of the mask / Jacobian chains
#define GMPC_FZ_MAX_T 32      // horizon limit
#define GMPC_FZ_MAX_HALVINGS 16
#define GMPC_FZ_LHM (GMPC_MAX_LAYERS - 1)   // hidden layers of one MLP at most

// box QP of the control-limited backward pass: projected-Newton iterations per QP at most, the Armijo
// constant and the number of step sizes 1, 1/2, ... tried per iteration
#define GMPC_BOX_QP_ITERS 40
#define GMPC_BOX_ARMIJO 0.1f
#define GMPC_BOX_QP_HALVINGS 16
#define GMPC_BOX_MAX_M 32

struct FusedSolveArgs {
  int n, m, T, k_max;             // k_max: step sizes alpha_0 / 2^k, k < k_max, that stay above alpha_min
  MlpDesc dyn, cost;              // W / WT / b of both MLPs (WT: the transposed copies gmpc_set_params builds)
  const float* mpc_w;
  gmpc_ilqr_opts opts;
  const float* x0;                // [B][n]
  const float* U_init;            // [B][T][m]
  const float* goal_in;           // [B][T+1][n]
  // ctx state the solve leaves behind (gmpc_bilevel_grad / gmpc_debug_buffer read it)
  float *X, *U, *goal, *AB, *QT, *qT, *K, *k, *grad, *adj;
  float *obj, *alpha, *obj_step, *U_step;
  int* iters;
  float* cand;                    // [B][GMPC_FZ_NC][(T+1) n + T m] candidate trajectories of the line search
  // caller outputs (any may be null)
  float *oX, *oU, *oobj, *ograd, *oadj;
  int* oiters;
};

// what the box solve takes on top: bounds [m] (null: unbounded on that side) and where its QPs report
struct BoxSolveArgs {
  const float *u_lo, *u_hi;
  float* count;                   // [B][2]: QPs of the solve that hit the iteration cap, QP iterations of the solve
  float* iters;                   // [B][T]: QP iterations of each step of the last backward pass
  float* clamped;                 // [B][T][m]: 1.0 where the control is in the final clamped set of that pass
};

// LDS bytes of the kernel for a shape (the largest of its phases; box: with the QP workspace and the bounds)
size_t gmpc_fused_lds_bytes(int n, int m, int T, bool box = false);
void gmpc_launch_ilqr_fused(const FusedSolveArgs& a, int B, hipStream_t s);
void gmpc_launch_ilqr_box(const FusedSolveArgs& a, const BoxSolveArgs& x, int B, hipStream_t s);
