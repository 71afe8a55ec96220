// The DDP line search as rounds of speculative candidates: the work list of a round (k_ls_init, k_ls_place), the
// decision and commit (k_ls_decide), the plan that says once per solve which kernels evaluate the candidates, and the
// launcher that enqueues the rounds.  The candidate kernels themselves are k_traj<true> (gmpc_traj.hip, any network
// shape), k_traj_rw<true> (gmpc_traj_rw.hip), k_ls16 and k_ls32 (gmpc_ls16.hip, gmpc_ls32.hip); what they share is
// gmpc_ls_common.h.
//
// Reference arithmetic: trajax line_search_ddp as called from policy/optimizers.py:19.
#include "gmpc_ls_common.h"
#include "gmpc_launch.h"
#include <cstdlib>
#include <cstring>

// ------------------------------------------------------------------------------------------------
// Round-based backtracking line search (trajax line_search_ddp: alpha = alpha_0, alpha_0/2, ... while
// alpha > alpha_min, the first candidate whose objective decreases is taken).  The halvings of one
// trajectory are independent rollouts, so a round evaluates several of them speculatively
// (one of the candidate kernels over a work list of (trajectory, halving count) candidates) and k_ls_decide picks,
// per trajectory, the LARGEST accepted step of the round -- the candidate the sequential loop would
// have stopped at -- commits it, or queues the next 4 halvings (8 from the third round on).  The first round of a trajectory
// covers the halvings up to the one its previous line search accepted (1 candidate for a
// well-conditioned problem that takes full steps, up to 8 for one that backtracks deeply), so the
// rollouts stay close to the sequential loop's count while the launches drop from up to 15
// dependent rollouts to 1-3 rounds.  Nothing is read back by the host.
// ------------------------------------------------------------------------------------------------
#define GMPC_LS_NEXT 4   // candidates queued per trajectory after a round without an accepted step

__global__ void k_ls_init(int B, const int* active, float alpha_0, float alpha_min, int k_max, int first_min, int* iters,
                          int* run, int* cnt, int* kfirst, const int* prevk, float* alpha, float* U_step,
                          float* obj_step) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  cnt[b] = 0;
  if (active != nullptr && active[b] == 0) { run[b] = 0; return; }
  iters[b] += 1;
  if (alpha_0 > alpha_min) {
    int R = prevk[b] + 1;
    R = R < first_min ? first_min : R;      // (first_min >= 1: see gmpc_ls_plan)
    R = R > GMPC_LS_ITEMS ? GMPC_LS_ITEMS : R;
    R = R > k_max ? k_max : R;
    run[b] = 1;
    cnt[b] = R;
    kfirst[b] = 0;
  } else {
    run[b] = 0;
    alpha[b] = alpha_0;
    U_step[b] = 0.f;
    obj_step[b] = 0.f;
  }
}

// Work list of a round, ordered by candidate number first and trajectory second: the four slots of a
// k_traj<true> workgroup then hold the SAME halving count of four trajectories.  Large steps are
// rejected early in the horizon (their running cost passes the objective to beat within a few
// steps), and a workgroup whose four candidates are all dead stops -- which only happens when
// candidates of similar fate sit together.  One workgroup; cnt[b] candidates for trajectory b.
__global__ __launch_bounds__(1024) void k_ls_place(int B, const int* cnt, const int* kfirst, int* item_b,
                                                   int* item_k, int* slot, int* count, int* total,
                                                   int* round_total) {
  __shared__ int s_n[GMPC_LS_ITEMS], s_base[GMPC_LS_ITEMS], s_fill[GMPC_LS_ITEMS];
  const int tid = threadIdx.x;
  if (tid < GMPC_LS_ITEMS) { s_n[tid] = 0; s_fill[tid] = 0; }
  __syncthreads();
  for (int b = tid; b < B; b += blockDim.x) {
    const int c = cnt[b];
    for (int j = 0; j < c; ++j) atomicAdd(&s_n[j], 1);
  }
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int j = 0; j < GMPC_LS_ITEMS; ++j) { s_base[j] = acc; acc += s_n[j]; }
    *count = acc;
    *total += acc;          // candidate rollouts since the solve began (one workgroup: no race)
    *round_total += acc;
  }
  __syncthreads();
  for (int b = tid; b < B; b += blockDim.x) {
    const int c = cnt[b], k0 = kfirst[b];
    for (int j = 0; j < c; ++j) {
      const int pos = s_base[j] + atomicAdd(&s_fill[j], 1);
      item_b[pos] = b;
      item_k[pos] = k0 + j;
      slot[b * GMPC_LS_ITEMS + j] = pos;
    }
  }
}

struct LsDecideArgs {
  int n, m, T, Lh, k_max;
  int next;              // candidates queued for the next round when this one accepts nothing
  float alpha_0;
  const int* slot; int* cnt; int* kfirst; int* prevk; int* run;
  const float* objc; const float* Xc; const float* Uc; const uint32_t* maskc;
  float* X; float* U; uint32_t* masks;
  float* obj; float* obj_step; float* U_step; float* alpha;
  int* stats;            // LsWork::counts + GMPC_LS_ROUNDS_MAX + 1
};

__global__ __launch_bounds__(GMPC_THREADS) void k_ls_decide(LsDecideArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (a.run[b] == 0) return;
  __shared__ int s_acc;
  __shared__ float s_us[GMPC_THREADS / 64];
  const int* sl = a.slot + (size_t)b * GMPC_LS_ITEMS;
  __shared__ int s_item;
  if (tid == 0) {
    float oo = a.obj[b];
    if (isnan(oo)) oo = INFINITY;
    const int R = a.cnt[b], k0 = a.kfirst[b];
    int acc = -1;
    float on_acc = 0.f;
    for (int j = 0; j < R; ++j) {
      float on = a.objc[sl[j]];
      if (isnan(on)) on = oo;
      if (on < oo) { acc = j; on_acc = on; break; }
    }
    s_item = acc >= 0 ? sl[acc] : 0;
    auto halved = [&](int k) { return ls_alpha(a.alpha_0, k); };
    if (acc >= 0) {
      a.obj[b] = on_acc;
      a.obj_step[b] = fabsf(on_acc - oo);
      a.alpha[b] = halved(k0 + acc + 1);
      a.prevk[b] = k0 + acc;
      a.run[b] = 0;
      a.cnt[b] = 0;
      atomicAdd(a.stats + min(k0 + acc, 15), 1);
      atomicMax(a.stats + 17, k0 + acc);       // deepest halving accepted since the solve began
    } else if (k0 + R >= a.k_max) {      // every step size down to alpha_min failed
      a.alpha[b] = halved(a.k_max);
      a.U_step[b] = 0.f;
      a.obj_step[b] = 0.f;
      a.prevk[b] = a.k_max - 1;
      a.run[b] = 0;
      a.cnt[b] = 0;
      atomicAdd(a.stats + 16, 1);
    } else {                               // queue the next GMPC_LS_NEXT halvings (k_ls_place)
      // (round 4, measured and not kept: a second round that reaches the deepest halving any trajectory of the batch
      // has accepted so far -- the third round it was meant to remove only exists in a solve's first iteration, and
      // the longer second round cost 0.2 ms per iteration)
      const int left = a.k_max - (k0 + R);
      a.cnt[b] = left < a.next ? left : a.next;
      a.kfirst[b] = k0 + R;
    }
    s_acc = acc;
  }
  __syncthreads();
  const int acc = s_acc;
  if (acc < 0) return;
  // commit the accepted candidate as the new iterate
  const size_t it = (size_t)s_item;
  const int n = a.n, m = a.m, T = a.T;
  float* Xd = a.X + (size_t)b * (T + 1) * n;
  const float* Xs = a.Xc + it * (T + 1) * n;
  for (int e = n + tid; e < (T + 1) * n; e += blockDim.x) Xd[e] = Xs[e];
  float us = 0.f;
  float* Ud = a.U + (size_t)b * T * m;
  const float* Us = a.Uc + it * T * m;
  for (int e = tid; e < T * m; e += blockDim.x) {
    const float un = Us[e], d = un - Ud[e];
    us = fmaf(d, d, us);
    Ud[e] = un;
  }
  const size_t mw = (size_t)T * a.Lh * GMPC_MW;
  uint32_t* Md = a.masks + (size_t)b * mw;
  const uint32_t* Ms = a.maskc + it * mw;
  for (size_t e = tid; e < mw; e += blockDim.x) Md[e] = Ms[e];
  us = wave_sum(us);
  if ((tid & 63) == 0) s_us[tid >> 6] = us;
  __syncthreads();
  if (tid == 0) a.U_step[b] = sqrtf((s_us[0] + s_us[1]) + (s_us[2] + s_us[3]));
}

// Host side ------------------------------------------------------------------------------------------------------
// halvings allowed by trajax' loop: candidate k runs while alpha_0 / 2^k > alpha_min (counted up to `cap`)
int gmpc_ls_halvings(float alpha_0, float alpha_min, int cap) {
  int k_max = 0;
  for (float al = alpha_0; al > alpha_min && k_max < cap; al *= 0.5f) ++k_max;
  return k_max;
}

int gmpc_ls_plan(const TrajArgs& a0, int ncu, bool custom_eval, LsPlan* p) {
  // the three switches, read here and nowhere else: once per plan, i.e. once per solve
  const char* form = getenv("GMPC_LS");               // "rw": k_traj_rw only; "ls16": never k_ls32
  const char* e16 = getenv("GMPC_LS16_SPLIT");        // work lists shorter than this stay on k_traj_rw
  const char* e32 = getenv("GMPC_LS32_SPLIT");        // work lists of at least this many items go to k_ls32 (0: never)
  const bool only_rw = form != nullptr && strcmp(form, "rw") == 0;
  const bool no_ls32 = only_rw || (form != nullptr && strcmp(form, "ls16") == 0);
  TrajArgs a = a0;
  const long all = (long)a.B * GMPC_LS_ITEMS;
  *p = LsPlan{};
  p->rw = !custom_eval && gmpc_traj_rw_shape(a);
  if (p->rw) {
    p->lds = gmpc_traj_rw_lds(a);
    p->aw = a.aw; p->pw = a.pw; p->sw0 = a.sw0; p->swl = a.swl;
  }
  // k_ls16: lists of 1537 candidates and more (shorter ones: 4 candidates per workgroup fill the chip sooner)
  p->ls16 = p->rw && !only_rw && gmpc_ls16_shape(a);
  if (p->ls16) p->split16 = e16 != nullptr && atoi(e16) > 0 ? atoi(e16) : 1537;
  // k_ls32: lists of at least 4097 candidates, more than one pass of k_ls16 over the 256 CUs (4096 candidates).  Measured
  // in round 4 at C3 (profiles/EXPERIMENTS.md): the 8192 candidates of a first round take one pass of k_ls32 0.79 ms
  // against 0.92 ms for two passes of k_ls16; a list of 4096 or fewer is one k_ls16 pass (0.46 ms) and would be half a
  // chip of k_ls32 for 0.79 ms.  The threshold is never below k_ls16's: the device guard (ls_round_form) then
  // partitions the counts, whatever the variables say.  (The tests set both to 1 to send every round to k_ls32.)
  const int s32 = e32 != nullptr ? atoi(e32) : 4097;
  if (p->ls16 && !no_ls32 && s32 > 0 && gmpc_ls32_shape(a)) {
    const int split32 = s32 > p->split16 ? s32 : p->split16;
    p->ls32 = all >= split32;
    if (p->ls32) p->split32 = split32;
  }
  p->k_max = gmpc_ls_halvings(a.alpha_0, a.alpha_min, 4096);
  // Size of the first round: one more candidate than the previous search accepted -- or, where a round of 16- or
  // 32-candidate workgroups runs anyway and has room, all GMPC_LS_ITEMS of them: a pass of k_ls32 over the chip holds
  // 8192 candidates (k_ls16: 4096) and takes the same time half empty.  At C3 the previous rule filled it to 7965 and
  // left ~10 trajectories per iteration whose step size had grown by more than four halvings with a THIRD round of
  // their own (a k_traj_rw pass, 0.2 - 0.4 ms for 80 candidates, in most iterations); with the full first round a
  // third round needs 13 halvings (20 of 102,400 searches).  Which candidate is accepted does not change.
  p->first_min = 1;
  if (p->ls16) {
    const long pass = p->ls32 ? (long)ncu * 32 : (long)ncu * 16;
    if (all >= p->split16 && all <= pass) p->first_min = GMPC_LS_ITEMS;
  }
  // worst case: a first round of first_min candidates, a second of GMPC_LS_NEXT, then GMPC_LS_ITEMS per round (a third
  // round is rare and every round enqueued costs four launches whether it finds work or not: the later rounds take all
  // they can hold; trajax' 15 step sizes are 4 rounds after a one-candidate first round, 3 after a full one)
  for (int left = p->k_max, r = 0; left > 0; ++r, ++p->rounds)
    left -= r == 0 ? p->first_min : r == 1 ? GMPC_LS_NEXT : GMPC_LS_ITEMS;
  return p->rounds > GMPC_LS_ROUNDS_MAX ? -1 : 0;
}

void gmpc_launch_linesearch(const TrajArgs& a0, const LsPlan& p, const LsWork& w, hipStream_t s, gmpc_ls_eval_fn eval,
                            void* user) {
  TrajArgs a = a0;
  a.aw = p.aw; a.pw = p.pw; a.sw0 = p.sw0; a.swl = p.swl;
  a.ls_split = p.split16; a.ls32_split = p.split32;
  hipLaunchKernelGGL(k_ls_init, dim3((a.B + 255) / 256), dim3(256), 0, s, a.B, a.active, a.alpha_0,
                     a.alpha_min, p.k_max, p.first_min, a.iters, w.run, w.cnt, w.kfirst, w.prevk, a.alpha, a.U_step,
                     a.obj_step);
  for (int r = 0; r < p.rounds; ++r) {
    hipLaunchKernelGGL(k_ls_place, dim3(1), dim3(1024), 0, s, a.B, w.cnt, w.kfirst, w.item_b[0], w.item_k[0],
                       w.slot, w.counts + r, w.counts + GMPC_LS_ROUNDS_MAX,
                       w.counts + GMPC_LS_ROUNDS_MAX + 1 + 24 + (r < GMPC_LS_STATS - 24 ? r : GMPC_LS_STATS - 25));
    a.item_b = w.item_b[0]; a.item_k = w.item_k[0]; a.nitems = w.counts + r; a.objc = w.objc;
    const long max_items = (long)a.B * (r == 1 ? GMPC_LS_NEXT : GMPC_LS_ITEMS);
    const int lsgrid = (int)((max_items + GMPC_TB - 1) / GMPC_TB);
    if (eval)
      eval(user, a, (int)max_items, s);
    else if (p.rw) {
      // three forms, each launch returns at once when the round's count is another form's (ls_round_form): 4
      // candidates per workgroup for short lists, 16 up to one pass over the chip, two groups of 16 beyond
      gmpc_launch_traj_rw(a, true, lsgrid, p.lds, s);
      if (p.ls16) gmpc_launch_ls16(a, max_items, s);
      if (p.ls32) gmpc_launch_ls32(a, max_items, s);
    } else
      gmpc_launch_traj(a, true, lsgrid, s);
    LsDecideArgs d;
    d.n = a.n; d.m = a.m; d.T = a.T; d.Lh = a.dyn.L - 1; d.k_max = p.k_max;
    d.next = r == 0 ? GMPC_LS_NEXT : GMPC_LS_ITEMS;      // size of round r + 1
    d.alpha_0 = a.alpha_0;
    d.slot = w.slot; d.cnt = w.cnt; d.kfirst = w.kfirst; d.prevk = w.prevk; d.run = w.run;
    d.objc = w.objc; d.Xc = a.Xc; d.Uc = a.Uc; d.maskc = a.maskc;
    d.X = a.X; d.U = a.Uio; d.masks = a.masks;
    d.obj = a.obj; d.obj_step = a.obj_step; d.U_step = a.U_step; d.alpha = a.alpha;
    d.stats = w.counts + GMPC_LS_ROUNDS_MAX + 1;
    hipLaunchKernelGGL(k_ls_decide, dim3(a.B), dim3(GMPC_THREADS), 0, s, d);
  }
}
