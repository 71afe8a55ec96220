"""NumPy restatement of the sample-efficient cross-entropy method (gmpc_icem_solve; Pinneri et
al., CoRL 2020) on top of cem_ref, in fp32 or fp64 (TEST INFRASTRUCTURE).  Per problem b and iteration it, a pool of
R = N_it + c + a rows:

  fresh rows     r < N_it: u = clamp(std zt + mean) with cem_ref's normals of sample index r; zt = z when noise_beta == 0
                 or T < 2, otherwise the coloured sum of the row's T normals z_k = z[k m + j] (colour)
  carried rows   the first c rows of the keep buffer (c = carry_in in a call's first iteration, num_keep afterwards)
  the mean       one row clamp(mean), in the call's last iteration with add_mean
  N_it           max(floor(n_it), min(N, 2 E)), n_0 = N, n_{k+1} = n_k / decay in float64 (sample_counts)
  elites         the E smallest by (cost, pool row), NaN as +inf; cem_ref.update's sums in rank order; a problem
                 without a finite cost keeps mean and std
  keep           the controls of ranks 0 .. num_keep-1;  best: rank 0 where strictly cheaper than the best so far
  returned U     best_U where return_best and best_cost is finite, the final mean otherwise
"""

import numpy as np

import cem_ref as cr
import gan_mpc_oracle as orc

DEFAULTS = dict(noise_beta=2.0, evolution_smoothing=0.1, elite_portion=0.1, keep_portion=0.3, decay=1.25, max_iter=3,
                num_samples=100, seed=0, add_mean=True, return_best=True)
TIE = dict(num_keep=0, decay=1.0, noise_beta=0.0, add_mean=False, return_best=False)


def sample_counts(N, E, decay, max_iter, iter_offset=0):
    """N_it of the iterations iter_offset .. iter_offset + max_iter - 1 (decay as the fp32 the options carry)."""
    d = np.float64(np.float32(decay))
    nk = np.float64(N)
    out = []
    for it in range(iter_offset + max_iter):
        if it >= iter_offset:
            out.append(max(int(np.floor(nk)), min(N, 2 * E)))
        nk = nk / d
    return out


def colour_weights(T, noise_beta):
    """cw [T // 2 + 1] in float64 (the library rounds it to fp32)."""
    beta = np.float64(np.float32(noise_beta))
    Kf = T // 2
    w = np.ones(Kf + 1)
    for k in range(1, Kf + 1):
        w[k] = np.power(np.float64(k) / np.float64(T), -beta / 2.0)
    if Kf >= 1:
        w[0] = w[1]
    inner = [k for k in range(1, Kf + 1) if 2 * k < T]
    s2 = w[0] ** 2 + sum(2.0 * w[k] ** 2 for k in inner) + (w[Kf] ** 2 if T % 2 == 0 else 0.0)
    s = np.sqrt(s2)
    cw = np.zeros(Kf + 1)
    cw[0] = w[0] / s
    for k in inner:
        cw[k] = np.sqrt(2.0) * w[k] / s
    if T % 2 == 0:
        cw[Kf] = w[Kf] / s
    return cw


def basis(T, cw):
    """M [T][T] in float64 with zt = M z (rows: steps t, columns: the normals k)."""
    M = np.zeros((T, T))
    t = np.arange(T)
    M[:, 0] = cw[0]
    k = 1
    while 2 * k < T:
        ang = 2.0 * np.pi * ((k * t) % T) / T
        M[:, 2 * k - 1] = cw[k] * np.cos(ang)
        M[:, 2 * k] = cw[k] * np.sin(ang)
        k += 1
    if T % 2 == 0:
        M[:, T - 1] = cw[T // 2] * np.where(t % 2 == 1, -1.0, 1.0)
    return M


def _fma32(a, b, c):
    """fp32 fma: the product of two fp32 is exact in float64."""
    return (a.astype(np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def colour(z, cw32, dtype):
    """z [..., T, m] (axis -2: the normals k) -> zt [..., T, m] (axis -2: the steps t).  cw32: the fp32 table.  fp64:
    the exact basis; fp32: the library's order -- k ascending, fma, the angle 2 ((k t) mod T) / T in fp32."""
    dtype = np.dtype(dtype).type
    T = z.shape[-2]
    cw32 = np.asarray(cw32, np.float32)
    if dtype is np.float64:
        return np.einsum("tk,...kj->...tj", basis(T, cw32.astype(np.float64)), z)
    out = np.empty_like(z)
    for t in range(T):
        acc = cw32[0] * z[..., 0, :]
        k = 1
        while 2 * k < T:
            ang = np.float32(2 * ((k * t) % T)) / np.float32(T)
            c, s = np.float32(np.cos(np.pi * np.float64(ang))), np.float32(np.sin(np.pi * np.float64(ang)))
            inner = _fma32(z[..., 2 * k, :], s, z[..., 2 * k - 1, :] * c)
            acc = _fma32(inner, cw32[k], acc)
            k += 1
        if T % 2 == 0:
            acc = _fma32(z[..., T - 1, :], -cw32[k] if t % 2 else cw32[k], acc)
        out[..., t, :] = acc
    return out


def clamp(u, lo, hi):
    if lo is not None:
        u = np.where(u < lo, lo, u)
    if hi is not None:
        u = np.where(u > hi, hi, u)
    return u


def draw(mean, std, lo, hi, seed, it, N, noise_beta, dtype=np.float64):
    """The N fresh rows of every problem: mean, std (B, T, m) -> (B, N, T, m).  lo / hi: None or [m] in dtype."""
    dtype = np.dtype(dtype).type
    B, T, m = mean.shape
    if noise_beta == 0.0 or T < 2:
        return cr.draw(mean, std, lo, hi, seed, it, N, 0.0, dtype)
    cw32 = colour_weights(T, noise_beta).astype(np.float32)
    out = np.empty((B, N, T, m), dtype)
    for b in range(B):
        z = cr.normals(seed, it, b, np.arange(N), T * m, dtype).reshape(N, T, m)
        zt = colour(z, cw32, dtype)
        if dtype is np.float32:
            u = _fma32(zt, std[b].astype(dtype), mean[b].astype(dtype))
        else:
            u = std[b].astype(dtype) * zt + mean[b].astype(dtype)
        out[b] = clamp(u, lo, hi)
    return out


def elite_counts(kw):
    N = int(kw["num_samples"])
    E = int(kw["num_elites"]) if "num_elites" in kw else int(N * kw["elite_portion"])
    nk = int(kw["num_keep"]) if "num_keep" in kw else int(E * kw["keep_portion"])
    return N, E, nk


def icem(pb, dtype, lo, hi, kwargs=None, trace=None, init_std=None, iter_offset=0, U_init=None, state=None,
         carry_in=None):
    """The whole solve on the problem pb (cast to dtype).  kwargs: DEFAULTS' keys, or num_elites / num_keep instead of
    the portions.  state: dict(keep, best_U, best_cost) of an earlier call (carry_in: default num_keep with a state, 0
    without).  trace: a list that receives one dict per iteration (pool (B, R, T, m), costs (B, R), elites, N_it,
    mean, std, keep, best_cost after the update).  -> dict(X, U, obj, mean, std, state)."""
    dtype = np.dtype(dtype).type
    kw = dict(DEFAULTS)
    kw.update(kwargs or {})
    p = orc.cast_problem(pb, dtype)
    N, E, nk = elite_counts(kw)
    K = int(kw["max_iter"])
    mean = (p["U"] if U_init is None else np.asarray(U_init)).astype(dtype).copy()
    B, T, m = mean.shape
    lo_v = None if lo is None else np.broadcast_to(np.asarray(lo, dtype), (m,))
    hi_v = None if hi is None else np.broadcast_to(np.asarray(hi, dtype), (m,))
    if init_std is None:
        std = np.broadcast_to((np.asarray(hi_v, np.float32) - np.asarray(lo_v, np.float32)) / np.float32(2),
                              (B, T, m)).astype(dtype)
    else:
        std = np.broadcast_to(np.asarray(init_std, dtype), (B, T, m)).astype(dtype)
    if state is None:
        keep, best_U, best_cost = np.zeros((B, nk, T, m), dtype), np.zeros((B, T, m), dtype), np.full(B, np.inf, dtype)
        carry_in = 0 if carry_in is None else carry_in
    else:
        keep, best_U = state["keep"].astype(dtype).copy(), state["best_U"].astype(dtype).copy()
        best_cost = state["best_cost"].astype(dtype).copy()
        carry_in = nk if carry_in is None else carry_in
    counts = sample_counts(N, E, kw["decay"], K, iter_offset)
    for i in range(K):
        c = carry_in if i == 0 else nk
        rows = [draw(mean, std, lo_v, hi_v, int(kw["seed"]), iter_offset + i, counts[i], kw["noise_beta"], dtype)]
        if c:
            rows.append(clamp(keep[:, :c], lo_v, hi_v))
        if kw["add_mean"] and i == K - 1:
            rows.append(clamp(mean, lo_v, hi_v)[:, None])
        pool = np.concatenate(rows, axis=1)
        costs = cr.sample_costs(p, pool)
        nmean, nstd, el = cr.update(pool, costs, mean, std, E, kw["evolution_smoothing"], dtype)
        top = costs[np.arange(B), el[:, 0]]
        alive = np.isfinite(top)
        mean = np.where(alive[:, None, None], nmean, mean)
        std = np.where(alive[:, None, None], nstd, std)
        keep = np.stack([pool[b][el[b, :nk]] for b in range(B)]).reshape(B, nk, T, m)
        with np.errstate(invalid="ignore"):
            better = top < best_cost
        best_cost = np.where(better, top, best_cost)
        best_U = np.where(better[:, None, None], pool[np.arange(B), el[:, 0]], best_U)
        if trace is not None:
            trace.append(dict(pool=pool, costs=costs, elites=el, N_it=counts[i], mean=mean.copy(), std=std.copy(),
                              keep=keep.copy(), best_cost=best_cost.copy()))
    give = np.isfinite(best_cost) if kw["return_best"] else np.zeros(B, bool)
    U = np.where(give[:, None, None], best_U, mean)
    with np.errstate(all="ignore"):
        X = orc.rollout(p["dyn"], U, p["x0"])
        obj = np.sum(orc.evaluate(p["cmlp"], p["mpc_w"], p["goal"], X, U), axis=1)
    return dict(X=X, U=U, obj=obj, mean=mean, std=std, state=dict(keep=keep, best_U=best_U, best_cost=best_cost))


def decided(tr32, tr64, E, nk, margin=1e-5):
    """cem_ref.decided extended to the pool: (iterations, B) bool.  Problem b is decided through iteration i when, at
    every iteration <= i, the fp32 and the fp64 run pick the same elite set and the same kept rows in the same order,
    and the fp64 costs leave a relative gap above `margin` at the elite cut (between the E-th and the (E+1)-th
    smallest) and between every two neighbours among the num_keep + 1 smallest (the keep cut, and the order of the
    kept rows, on which the later pools' rows depend)."""
    out, ok = [], None
    for a, b in zip(tr32, tr64):
        same = np.array([set(x) == set(y) and list(x[:nk]) == list(y[:nk]) for x, y in zip(a["elites"], b["elites"])])
        c = np.sort(np.where(np.isnan(b["costs"]), np.inf, b["costs"]), axis=1)
        gap = np.full(c.shape[0], np.inf)
        cuts = list(range(min(nk, c.shape[1] - 1))) + ([E - 1] if c.shape[1] > E else [])
        with np.errstate(all="ignore"):
            for i in cuts:
                gap = np.minimum(gap, (c[:, i + 1] - c[:, i]) / np.abs(c[:, i]))
        now = same & (gap > margin)
        ok = now if ok is None else ok & now
        out.append(ok.copy())
    return np.array(out)
