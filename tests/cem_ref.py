"""NumPy restatement of the cross-entropy method solver (gmpc_cem_solve; trajax `cem`) on the
oracle's objective, in fp32 or fp64 (TEST INFRASTRUCTURE).  Per problem b and iteration it:

  z[s][t][j]   standard normal: Philox4x32-10 under the key (seed low word, seed high word) at the counter
               (e >> 2, s, b, it), output word e & 3, e = t m + j; u_i = ((r_i >> 9) 2 + 1) 2^-24; Box-Muller on
               (u0, u1) -> words 0 / 1 (cos / sin) and on (u2, u3) -> words 2 / 3
  zt           z smoothed along time: zt_0 = z_0, zt_t = beta zt_{t-1} + sqrt(1 - beta^2) z_t
  u            clamp(std zt + mean, lo, hi) by two selects (a NaN stays a NaN)
  cost_s       orc.objective of the sample
  elites       the E smallest by (cost, sample index), NaN as +inf
  update       sums over the elites in rank order: new_mean = sum u / E, new_std = sqrt(sum (u - new_mean)^2 / E);
               mean <- gamma mean + (1 - gamma) new_mean, std likewise
"""

import numpy as np

import gan_mpc_oracle as orc

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF

DEFAULTS = dict(sampling_smoothing=0.0, evolution_smoothing=0.1, elite_portion=0.1, max_iter=10, num_samples=400,
                seed=0)


def philox(counter, key):
    """Philox4x32-10: counter = 4 uint32 arrays (broadcastable), key = 2 -> 4 uint32 arrays."""
    c = [np.asarray(x, np.uint64) & MASK for x in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)) & MASK, p1 & MASK,
             ((p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)) & MASK, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [x.astype(np.uint32) for x in c]


def uniforms(r, dtype):
    """((r >> 9) 2 + 1) 2^-24: exact in fp32, never 0 or 1."""
    return (((np.asarray(r, np.uint32) >> np.uint32(9)).astype(np.int64) * 2 + 1).astype(dtype)
            * dtype(2.0 ** -24))


def normals(seed, it, b, s, count, dtype=np.float64):
    """z[s][e], e < count, of problem b at iteration it; s: the sample indices (any int array) -> s.shape + (count,)."""
    dtype = np.dtype(dtype).type
    s = np.asarray(s)
    e = np.arange(count)
    r = philox((e >> 2, s[..., None], b, it), (seed & MASK, (seed >> 32) & MASK))
    w = e & 3
    ra = np.where(w & 2, r[2], r[0])
    rb = np.where(w & 2, r[3], r[1])
    ua, ub = uniforms(ra, dtype), uniforms(rb, dtype)
    rad = np.sqrt(dtype(-2.0) * np.log(ua))
    ang = dtype(2.0 * np.pi) * ub
    return np.where(w & 1, rad * np.sin(ang), rad * np.cos(ang)).astype(dtype)


def smooth(z, beta, dtype):
    """z [..., T, m] smoothed along T."""
    dtype = np.dtype(dtype).type
    if beta == 0.0:
        return z
    bt, cb = dtype(np.float32(beta)), dtype(np.sqrt(np.float32(1.0) - np.float32(beta) * np.float32(beta)))
    out = z.copy()
    for t in range(1, z.shape[-2]):
        out[..., t, :] = bt * out[..., t - 1, :] + cb * z[..., t, :]
    return out


def draw(mean, std, lo, hi, seed, it, N, beta=0.0, dtype=np.float64):
    """The N samples of every problem: mean, std (B, T, m) -> (B, N, T, m).  lo / hi: None or [m]."""
    dtype = np.dtype(dtype).type
    B, T, m = mean.shape
    out = np.empty((B, N, T, m), dtype)
    for b in range(B):
        z = smooth(normals(seed, it, b, np.arange(N), T * m, dtype).reshape(N, T, m), beta, dtype)
        u = std[b].astype(dtype) * z + mean[b].astype(dtype)
        if lo is not None:
            u = np.where(u < np.asarray(lo, dtype), np.asarray(lo, dtype), u)
        if hi is not None:
            u = np.where(u > np.asarray(hi, dtype), np.asarray(hi, dtype), u)
        out[b] = u
    return out


def sample_costs(pb, samples):
    """orc.objective of every sample: samples (B, N, T, m) -> (B, N), in the dtype of pb."""
    B, N, T, m = samples.shape
    x0 = np.repeat(pb["x0"], N, axis=0)
    goal = np.repeat(pb["goal"], N, axis=0)
    with np.errstate(all="ignore"):
        c = orc.objective(pb["dyn"], pb["cmlp"], pb["mpc_w"], goal, samples.reshape(B * N, T, m).astype(x0.dtype), x0)
    return c.reshape(B, N)


def elites_of(costs, E):
    """(B, N) -> (B, E) sample indices: the E smallest by (cost, index), a NaN cost as +inf."""
    c = np.where(np.isnan(costs), np.inf, costs)
    return np.argsort(c, axis=1, kind="stable")[:, :E]


def update(samples, costs, mean, std, E, gamma, dtype=np.float64, elites=None):
    """One refit: -> (mean, std, elites).  Sequential sums in rank order, in `dtype`; elites: use these instead of
    selecting them from `costs`."""
    dtype = np.dtype(dtype).type
    el = elites_of(costs, E) if elites is None else np.asarray(elites)
    B = samples.shape[0]
    u = np.stack([samples[b][el[b]] for b in range(B)]).astype(dtype)      # (B, E, T, m)
    s = np.zeros_like(u[:, 0])
    for r in range(E):
        s = s + u[:, r]
    nm = s / dtype(E)
    ss = np.zeros_like(s)
    for r in range(E):
        d = u[:, r] - nm
        ss = ss + d * d
    ns = np.sqrt(ss / dtype(E))
    g = dtype(np.float32(gamma))
    g1 = dtype(np.float32(1.0) - np.float32(gamma))
    return g * mean.astype(dtype) + g1 * nm, g * std.astype(dtype) + g1 * ns, el


def cem(pb, dtype, lo, hi, kwargs=None, trace=None, init_std=None, iter_offset=0, U_init=None):
    """The whole solve on the problem pb (cast to dtype).  kwargs: DEFAULTS' keys, or num_elites instead of
    elite_portion.  trace: a list that receives one dict per iteration (samples, costs, elites, mean, std after the
    update).  -> dict(X, U, obj, std)."""
    dtype = np.dtype(dtype).type
    kw = dict(DEFAULTS)
    kw.update(kwargs or {})
    p = orc.cast_problem(pb, dtype)
    N = int(kw["num_samples"])
    E = int(kw["num_elites"]) if "num_elites" in kw else int(N * kw["elite_portion"])
    mean = (p["U"] if U_init is None else np.asarray(U_init)).astype(dtype).copy()
    B, T, m = mean.shape
    lo_v = None if lo is None else np.broadcast_to(np.asarray(lo, dtype), (m,))
    hi_v = None if hi is None else np.broadcast_to(np.asarray(hi, dtype), (m,))
    if init_std is None:
        std = np.broadcast_to((np.asarray(hi_v, np.float32) - np.asarray(lo_v, np.float32)) / np.float32(2),
                              (B, T, m)).astype(dtype)
    else:
        std = np.broadcast_to(np.asarray(init_std, dtype), (B, T, m)).astype(dtype)
    for i in range(int(kw["max_iter"])):
        u = draw(mean, std, lo_v, hi_v, int(kw["seed"]), iter_offset + i, N, kw["sampling_smoothing"], dtype)
        c = sample_costs(p, u)
        mean, std, el = update(u, c, mean, std, E, kw["evolution_smoothing"], dtype)
        if trace is not None:
            trace.append(dict(samples=u, costs=c, elites=el, mean=mean.copy(), std=std.copy()))
    X = orc.rollout(p["dyn"], mean, p["x0"])
    obj = np.sum(orc.evaluate(p["cmlp"], p["mpc_w"], p["goal"], X, mean), axis=1)
    return dict(X=X, U=mean, obj=obj, std=std)


def decided(tr32, tr64, E, margin=1e-5):
    """(iterations, B) bool: problem b is decided through iteration i when, at every iteration <= i, the fp32 and the
    fp64 run pick the same elite set and the fp64 costs leave a relative gap above `margin` between the E-th and the
    (E+1)-th smallest."""
    out = []
    ok = None
    for a, b in zip(tr32, tr64):
        same = np.array([set(x) == set(y) for x, y in zip(a["elites"], b["elites"])])
        c = np.sort(np.where(np.isnan(b["costs"]), np.inf, b["costs"]), axis=1)
        if c.shape[1] > E:
            gap = (c[:, E] - c[:, E - 1]) / np.abs(c[:, E - 1])
        else:
            gap = np.full(c.shape[0], np.inf)
        now = same & (gap > margin)
        ok = now if ok is None else ok & now
        out.append(ok.copy())
    return np.array(out)
