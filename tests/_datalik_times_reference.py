"""The data log-likelihood at arbitrary observation times in extended precision: the yardstick of the tests of
`data_loglik_times_kernel`.

Per trajectory, the AUGMENTED CHAIN is its filter records t_0 .. t_{n-1} (n = n_save on a fixed grid, NSAVED[i] with the times
T[:, i] after an adaptive solve) with one extra node per observation time tau_j that equals none of its save times.  For
t_k < tau_j < t_{k+1} the node is the filter's prediction from record k over h1 = tau_j - t_k, formed in the coordinates
preconditioned with P(h1) with sigma2 = DIFFUSION[k + 1]:

    m = P^-1 A P m_k,     C = P^-1 (A P Sigma_k P A' + sigma2 Q) P^-1

(what `oracle.dense_output(..., smoothed=False)` forms).  Its own diffusion slot is DIFFUSION[k + 1] as well, so both sub-steps of
a split interval use it; a node that follows another node of the same interval is predicted from record k too.  The likelihood is
`_datalik_reference.sweep` -- imported, not copied -- over that chain with the nodes and the hit saves as observed positions.
tau_j == t_k is observed at save k (of repeated times the last copy: xi is the same at all).  A tau_j above the trajectory's last
save gives NaN for that trajectory; tau_1 < t_0 is an error.

The nodes are formed in `dtype` and handed to the sweep as they are (longdouble nodes are not rounded to float64).  With
dtype=np.float64 the whole evaluation, prediction included, is the plain numpy one that calibrates the tolerance."""
import numpy as np

import _datalik_reference as dr
from _datalik_reference import orc  # noqa: F401

KEYS = dr.KEYS
DEVICE_FACTOR = dr.DEVICE_FACTOR
# Worst error / unit bound of the numpy FLOAT64 evaluation against the longdouble reference over the inputs of
# tests/test_datalik_times_emul.py and of tests/test_gpu_datalik_times.py (the latter on oracle solves of the same problems):
# measured 0.0035 (rounded up: C_MEASURED), which is below the 0.03 of the save path, so 0.03 stays.
# tests/test_datalik_times_reference.py::test_float64_numpy_evaluation_calibrates_the_tolerance repeats the measurement.
C_MEASURED = 0.005
C_NUMPY = max(dr.C_NUMPY, C_MEASURED)


def _pack(Cm):
    """[Nb, D, D] -> packed lower triangle [TRI, Nb]."""
    D = Cm.shape[-1]
    il = np.tril_indices(D)
    return np.ascontiguousarray(Cm[:, il[0], il[1]].T)


def predict_node(mean_k, cov_k, s2, h1, d, q, dtype):
    """The filter's prediction from the records (mean_k [D, Nb], cov_k [TRI, Nb]) over h1 with diffusion s2 [Nb], in `dtype`:
    (mean [D, Nb], cov_tril [TRI, Nb])."""
    D = d * (q + 1)
    dt = np.dtype(dtype).type
    A, Q = dr.prior(d, q, dtype)
    P = dr.precond(np.float64(h1), d, q, dtype)
    Pi = dt(1) / P
    X = dr.unpack(cov_k, D, dtype) * P[:, None] * P[None, :]
    mt = mean_k.T.astype(dtype) * P
    B = A @ X @ A.T + s2.astype(dtype)[:, None, None] * Q
    B = (B + B.transpose(0, 2, 1)) / dt(2)
    m = (mt @ A.T) * Pi
    C = B * Pi[:, None] * Pi[None, :]
    return np.ascontiguousarray(m.T), _pack(C)


def augmented_chain(mean, cov_tril, diffusion, t, d, q, times, dtype=np.longdouble):
    """Chain of trajectories that share the save times t [n]: records mean [n, D, Nb], cov_tril [n, TRI, Nb], diffusion [n, Nb].
    Returns (mean, cov_tril, diffusion, t, saves) of the augmented chain -- arrays of `dtype`, t float64, saves the positions of
    the M observation times --, or None when the last time lies above t[n - 1]."""
    mean, cov_tril, diffusion = dr._records(mean, cov_tril, diffusion)
    t = np.asarray(t, np.float64)
    times = np.asarray(times, np.float64)
    n = len(t)
    assert n >= 1 and np.all(np.diff(t) >= 0) and np.all(np.diff(times) > 0) and np.all(np.isfinite(times))
    if times[0] < t[0]:
        raise ValueError("observation time before t0")
    if times[-1] > t[-1]:
        return None
    ms, cs, ds, ts, saves = [], [], [], [], []
    j = 0
    M = len(times)
    for k in range(n):
        ms.append(mean[k].astype(dtype)); cs.append(cov_tril[k].astype(dtype)); ds.append(diffusion[k].astype(dtype)); ts.append(t[k])
        last_copy = k == n - 1 or t[k + 1] != t[k]
        if j < M and times[j] == t[k] and last_copy:
            saves.append(len(ts) - 1)
            j += 1
        while j < M and k + 1 < n and t[k] < times[j] < t[k + 1]:
            m, c = predict_node(mean[k], cov_tril[k], diffusion[k + 1], times[j] - t[k], d, q, dtype)
            ms.append(m); cs.append(c); ds.append(diffusion[k + 1].astype(dtype)); ts.append(times[j])
            saves.append(len(ts) - 1)
            j += 1
    assert j == M, (j, M)
    # Slot s of the diffusion belongs to the step s - 1 -> s.  A node carries DIFFUSION[k + 1] and save k + 1 holds it already, so
    # every sub-step of a split interval uses it.
    return np.stack(ms), np.stack(cs), np.stack(ds), np.array(ts), saves


def _groups(t, nsaved, N):
    """Lists of trajectories that share their save times: [(t_i [n_i], [indices])]."""
    t = np.asarray(t, np.float64)
    if t.ndim == 1:
        return [(t, list(range(N)))]
    out = {}
    for i in range(N):
        ti = t[: int(nsaved[i]), i]
        out.setdefault(ti.tobytes(), (ti, []))[1].append(i)
    return list(out.values())


def _per_group(fn, mean, cov_tril, diffusion, t, d, q, times, comps, y, r, nsaved, dtype):
    mean, cov_tril, diffusion = dr._records(mean, cov_tril, diffusion)
    N = mean.shape[-1]
    M, o = len(times), len(comps)
    y = dr._values(y, N, M, o)
    out = {k: np.full(N, np.nan, np.dtype(dtype)) for k in KEYS}
    for ti, idx in _groups(t, nsaved, N):
        n = len(ti)
        if n < 1:
            continue
        ch = augmented_chain(mean[:n][:, :, idx], cov_tril[:n][:, :, idx], diffusion[:n][:, idx], ti, d, q, times, dtype)
        if ch is None:
            continue
        res = fn(ch[0], ch[1], ch[2], ch[3], d, q, ch[4], comps, y[idx], r)
        for k in KEYS:
            out[k][idx] = res[k]
    return out


def evaluate(mean, cov_tril, diffusion, t, d, q, times, comps, y, r, nsaved=None, dtype=np.longdouble):
    """dict with loglik, mahalanobis [N] in `dtype`.  t [n] (a fixed grid) or [n, N] with nsaved [N] (an adaptive solve)."""
    fn = lambda *a: dr.sweep(*a, dtype)  # noqa: E731
    return _per_group(fn, mean, cov_tril, diffusion, t, d, q, times, comps, y, r, nsaved, dtype)


def unit_bound(mean, cov_tril, diffusion, t, d, q, times, comps, y, r, nsaved=None):
    """`_datalik_reference.unit_bound` over the augmented chain (float64 [N] per key; NaN where the reference is NaN)."""
    return _per_group(dr.unit_bound, mean, cov_tril, diffusion, t, d, q, times, comps, y, r, nsaved, np.float64)


def check(got, ref, bounds, factor=DEVICE_FACTOR, label=""):
    """Asserts |got - ref| <= factor C_NUMPY unit bound for both quantities; returns the ratios error / unit bound."""
    rt = dr.ratios(got, ref, bounds)
    for k in KEYS:
        assert rt[k] <= factor * C_NUMPY, (label, k, rt[k], factor * C_NUMPY)
    return rt


# ---- the inputs of tests/test_datalik_times_emul.py (and of the calibration in tests/test_datalik_times_reference.py) ------------

def adaptive_records(vf, alg, u0s, tspan, ps=None, repeat_at=(), drop_last=None, pad=2, **kw):
    """Oracle adaptive solves of the trajectories u0s written in the device layout of an adaptive solve: (mean [cap, D, N], cov_tril
    [cap, TRI, N], diffusion [cap, N], T [cap, N], NSAVED [N]); cap = the longest record count + pad, slots beyond a trajectory's
    own records hold NaN.  `repeat_at`: record indices planted again at the unchanged time (h = 0, as a rejected attempt leaves
    them).  `drop_last`: {trajectory: records dropped from its end} (a solve that stopped early)."""
    cols = []
    for i, u0 in enumerate(u0s):
        s = orc.solve(vf, alg, u0=u0, p=None if ps is None else ps[i], tspan=tspan, adaptive=True, **kw)
        D = s.d * (s.q + 1)
        il = np.tril_indices(D)
        mu, cov, t = list(s.means(False)), list(s.covs(False)), list(s.t)
        df = [0.0] + list(s.diffusions)
        for k in sorted(repeat_at, reverse=True):
            mu.insert(k + 1, mu[k]); cov.insert(k + 1, cov[k]); t.insert(k + 1, t[k]); df.insert(k + 1, df[k])
        cut = len(t) - (drop_last or {}).get(i, 0)
        cols.append((np.array(mu)[:cut], np.array(cov)[:cut][:, il[0], il[1]], np.array(df)[:cut], np.array(t)[:cut]))
    N = len(cols)
    cap = max(len(c[3]) for c in cols) + pad
    D, TRI = cols[0][0].shape[1], cols[0][1].shape[1]
    mean, covt = np.full((cap, D, N), np.nan), np.full((cap, TRI, N), np.nan)
    diff, T = np.full((cap, N), np.nan), np.full((cap, N), np.nan)
    nsaved = np.zeros(N, np.int32)
    for i, (m, c, f, t) in enumerate(cols):
        n = len(t)
        mean[:n, :, i], covt[:n, :, i], diff[:n, i], T[:n, i], nsaved[i] = m, c, f, t, n
    return mean, covt, diff, T, nsaved


def observations(mean, t, nsaved, times, comps, r, per_traj, seed):
    """y = the record means interpolated linearly at `times` (trajectory 0 when shared) plus seeded N(0, r) noise: [M, o] or
    [N, M, o].  Any values are a valid input of the pass."""
    rng = np.random.default_rng(seed)
    N = mean.shape[-1]
    t = np.asarray(t)
    y = np.zeros((N, len(times), len(comps)))
    for i in range(N if per_traj else 1):
        n = mean.shape[0] if nsaved is None else int(nsaved[i])
        ti = t[:n] if t.ndim == 1 else t[:n, i]
        for a, c in enumerate(comps):
            y[i, :, a] = np.interp(times, ti, np.nan_to_num(mean[:n, c, i]))
    y += rng.standard_normal(y.shape) * np.sqrt(np.asarray(r, float))[None, None, :]
    return np.ascontiguousarray(y) if per_traj else np.ascontiguousarray(y[0])


def _tile(arrs, N, seed):
    """`distinct` trajectories repeated to N whose means then differ per lane by a relative 1e-3 (every lane its own numbers)."""
    nd = arrs[0].shape[-1]
    reps = -(-N // nd)
    out = [np.ascontiguousarray(np.tile(a, reps)[..., :N]) for a in arrs]
    out[0] = out[0] * (1.0 + 1e-3 * np.random.default_rng(seed + 1).standard_normal((1, 1, N)))
    return out


def _fixed_case(field, alg, N, tgrid, times, comps, r, per_traj, seed, repeat_at=()):
    """Fixed grid: the records of `_datalik_reference._case`; `times(t)` maps the save times to the observation times."""
    c = dr._case(field, alg, N, tgrid, (0,), comps, r, per_traj, seed, repeat_at=repeat_at)
    tau = np.asarray(times(c["t"]), float)
    y = observations(c["mean"], c["t"], None, tau, comps, c["r"], per_traj, seed)
    return dict(mean=c["mean"], cov=c["cov"], diff=c["diff"], t=c["t"], nsaved=None, d=c["d"], q=c["q"], times=tau, comps=list(comps),
                y=y, r=c["r"])


def _ragged_case(field, alg, N, tspan, times, comps, r, per_traj, seed, distinct=5, scale=5e-2, repeat_at=(), drop_last=None, **kw):
    """Ragged grids: adaptive oracle solves of `distinct` perturbed initial values, tiled to N lanes."""
    vf = field if not isinstance(field, str) else orc.vector_field(field)
    nd = min(N, distinct)
    u0s = orc.ensemble_u0(vf.u0, nd, scale)
    mean, cov, diff, T, ns = _tile(adaptive_records(vf, alg, u0s, tspan, repeat_at=repeat_at, drop_last=drop_last, **kw), N, seed)
    ns = ns.astype(np.int32)
    tau = np.asarray(times(T[: ns[0], 0]), float)
    r = np.broadcast_to(np.asarray(r, float), (len(comps),)).copy()
    y = observations(mean, T, ns, tau, comps, r, per_traj, seed)
    return dict(mean=mean, cov=cov, diff=diff, t=T, nsaved=ns, d=vf.d, q=alg.order, times=tau, comps=list(comps), y=y, r=r)


def above_saves(t, seed=5):
    """One time per step of the saves t, 1e-6 to 1e-3 of the step above its left save (log-uniform, seeded), from step 1 on; steps
    of length zero (repeats) carry none."""
    t = np.asarray(t, float)
    k = np.array([a for a in range(1, len(t) - 1) if t[a + 1] > t[a]])
    f = 10.0 ** np.random.default_rng(seed).uniform(-6.0, -3.0, len(k))
    tau = t[k] + f * (t[k + 1] - t[k])
    return tau[np.concatenate([[True], np.diff(tau) > 0])]


def _build_cases():
    g = lambda n, h: np.arange(n) * h  # noqa: E731
    up, dn = (lambda x: np.nextafter(x, np.inf)), (lambda x: np.nextafter(x, -np.inf))  # noqa: E731
    c = {}
    # save 0, two times inside one step, a save, nextafter above a save, the last save
    c["lin1-ek0q1-N1-mixed"] = _fixed_case(dr._linear_field(1), orc.EK0(order=1), 1, g(5, 0.125),
                                           lambda t: [t[0], t[1] + 0.04, t[1] + 0.08, t[2], up(t[3]), t[4]], (0,), 1e-4, False, 1)
    # three times inside one step, nextafter below a save and the save itself; o = d, per-trajectory values, fixed diffusion
    c["fhn-ek1q1-fixed-N65-three-in-step"] = _fixed_case(
        "fhn", orc.EK1(order=1, diffusionmodel="fixed"), 65, g(17, 0.0625),
        lambda t: [t[5] + 0.2 * 0.0625, t[5] + 0.5 * 0.0625, t[5] + 0.9 * 0.0625, dn(t[8]), t[8]], (0, 1), (1e-3, 4e-3), True, 2)
    c["lv-ek0q3-N130-all-in-first-step"] = _fixed_case("lotka_volterra", orc.EK0(order=3), 130, g(33, 2.0 ** -5),
                                                       lambda t: t[0] + t[1] * np.array([0.1, 0.35, 0.6, 0.9]), (1,), 1e-2, False, 3)
    c["lv-ek1q3-map-N65-all-in-last-step"] = _fixed_case(
        "lotka_volterra", orc.EK1(order=3, diffusionmodel="fixedMAP"), 65, g(12, 0.0625),
        lambda t: t[-2] + 0.0625 * np.array([0.1, 0.5, 0.9]), (0, 1), 1e-2, True, 4)
    # (no time one ulp from a save here: with [t0, below t1, t3 + .03, t3 + .09, t6, above t6, t8] the numpy float64 evaluation
    # itself lies 3.7e7 unit bounds from the longdouble one on this field -- the host build 4.3e4 --, so the input is outside
    # what C_NUMPY speaks for; the other fields carry the nextafter times)
    c["lin4-ek0q2-N65-mixed-pertraj"] = _fixed_case(dr._linear_field(4), orc.EK0(order=2), 65, g(9, 0.125),
                                                    lambda t: [t[0], t[1] + 0.1, t[3] + 0.03, t[3] + 0.09, t[6], t[8]], (1, 3),
                                                    1e-3, True, 5)
    # a grid with repeated times (records 3 and 7 planted again): a time on the repeated save, times around it
    c["fhn-ek1q1-N65-repeat"] = _fixed_case("fhn", orc.EK1(order=1), 65, g(15, 0.0625),
                                            lambda t: [t[2] + 0.01, t[3], t[3] + 0.02, t[8], up(t[8]), dn(t[10]), t[-1]], (0, 1), 1e-3, False, 6,
                                            repeat_at=(3, 7))
    # ragged grids: save 0, two times in one step of lane 0, a save of lane 0 (inside a step of the others) and one ulp above it,
    # one ulp below a save of lane 0, the shared last save
    mid = lambda t: len(t) // 2  # noqa: E731
    two = lambda t: [t[4] + 0.3 * (t[5] - t[4]), t[4] + 0.7 * (t[5] - t[4])]  # noqa: E731
    mixed = lambda t: [t[0]] + two(t) + [t[mid(t)], up(t[mid(t)]), dn(t[mid(t) + 2]), t[-1]]  # noqa: E731
    mixed_up = lambda t: [up(t[2])] + two(t) + [t[mid(t)], up(t[mid(t)]), dn(t[mid(t) + 2]), t[-1]]  # noqa: E731
    # (order 5 without the pair {save, one ulp above it}: over a step of one ulp P(h) spans 1e88, and the numpy float64 evaluation
    # itself then lies 61 unit bounds from the longdouble one -- the host build 0.0046 --, outside what C_NUMPY speaks for; the
    # above-saves case below carries order 5 at 1e-6 to 1e-3 of a step)
    mixed_q5 = lambda t: [up(t[2])] + two(t) + [t[mid(t)], dn(t[mid(t) + 2]), t[-1]]  # noqa: E731
    c["lorenz-ek1q3-N130-ragged"] = _ragged_case("lorenz63", orc.EK1(order=3), 130, (0.0, 0.25), mixed, (0, 2), 1e-2, False, 7, dt=2.0 ** -6,
                                                 repeat_at=(2, 9))
    c["fhn-ek0q5-N65-ragged-pertraj"] = _ragged_case("fhn", orc.EK0(order=5), 65, (0.0, 1.0), mixed_q5, (0,), 1e-3, True, 8, dt=2.0 ** -5)
    c["lv-ek0q3-map-N65-ragged"] = _ragged_case("lotka_volterra", orc.EK0(order=3, diffusionmodel="fixedMAP"), 65, (0.0, 1.0), mixed,
                                                (0, 1), 1e-2, True, 9, dt=2.0 ** -5)
    # lanes 1, 6, 11, .. stop three records early: their records end before the last time
    c["lorenz-ek1q3-N65-ragged-short"] = _ragged_case("lorenz63", orc.EK1(order=3), 65, (0.0, 0.25), mixed_up, (0, 1, 2), 1e-2, False, 10,
                                                      dt=2.0 ** -6, drop_last={1: 3})
    # about one time per step, each 1e-6 to 1e-3 of the step above a save of lane 0 (seeded; none is the first of the set): the step
    # from such a node onto the save below it is the one that must not factor the node's prediction (datalik_times_kernels.h)
    c["lorenz-ek1q3-N65-ragged-above-saves"] = _ragged_case("lorenz63", orc.EK1(order=3), 65, (0.0, 0.5), above_saves, (0, 1, 2), 1e-4,
                                                            False, 11, dt=2.0 ** -7)
    c["fhn-ek0q5-N65-ragged-above-saves"] = _ragged_case("fhn", orc.EK0(order=5), 65, (0.0, 1.0), above_saves, (0, 1), 1e-3, True, 12,
                                                         dt=2.0 ** -5)
    return c


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _build_cases()
    return _CASES


def _args(c):
    return (c["mean"], c["cov"], c["diff"], c["t"], c["d"], c["q"], c["times"], c["comps"], c["y"], c["r"], c["nsaved"])


def run_reference(c, dtype=np.longdouble):
    return evaluate(*_args(c), dtype=dtype)


def case_bound(c):
    return unit_bound(*_args(c))


# ---- the problems of tests/test_gpu_datalik_times.py; the calibration runs them on oracle solves of a few trajectories -----------

def _late(lo, hi, M):
    """M times spread over [lo, hi] at irregular spacings (none a save time of an adaptive solve)."""
    x = np.linspace(0.0, 1.0, M) ** 1.1
    return lo + (hi - lo) * (0.013 + 0.97 * x)


# The times of the adaptive problems are per ensemble and fall where they fall in every trajectory's own grid.  The GPU tests repeat
# the calibration on the records they read: the numpy float64 evaluation must itself meet C_NUMPY there.  (With the last time of the
# Lotka-Volterra problem at 1.9898 it does not: on one of the device's 66 trajectories, whose last step is a fifth of its others with
# a diffusion 20 times theirs, numpy float64 lies 50 unit bounds -- 6.5e-8 absolute on 4.4 -- from the longdouble value, the host build
# 42; the unit bound is 1.3e-9 there.  The times end at 1.95 instead; "above-saves" covers times shortly above saves.)
GPU_PROBLEMS = {
    # name: (field, kind, order, diffusion, t1, adaptive, dt, times(t) -> [M], comps, r, per_traj)
    "lv-ek1q3-fixed": ("lotka_volterra", "EK1", 3, "dynamic", 2.0, False, 2.0 ** -4,
                       lambda t: [t[3], t[9] + 0.02, t[9] + 0.05, t[14] + 0.01, np.nextafter(t[20], -np.inf), t[25] + 0.03, t[31] + 0.06],
                       (0, 1), 1e-2, False),
    "lv-ek1q3-adaptive": ("lotka_volterra", "EK1", 3, "dynamic", 2.0, True, 2.0 ** -6, lambda t: _late(1.4, 1.95, 5), (1,), 1e-2, True),
    "lorenz-ek1q3-adaptive": ("lorenz63", "EK1", 3, "dynamic", 0.25, True, 2.0 ** -7, lambda t: _late(0.15, 0.25, 5), (0, 2), 1e-2, False),
    "lorenz-ek1q3-map-adaptive": ("lorenz63", "EK1", 3, "fixedMAP", 0.25, True, 2.0 ** -7, lambda t: _late(0.15, 0.25, 5), (0, 2), 1e-2,
                                  False),
    "fhn-ek0q5-adaptive": ("fhn", "EK0", 5, "dynamic", 1.0, True, 2.0 ** -5, lambda t: _late(0.6, 1.0, 4), (0, 1), 1e-3, False),
    "lorenz-ek1q3-adaptive-above-saves": ("lorenz63", "EK1", 3, "dynamic", 0.25, True, 2.0 ** -7, above_saves, (0, 1, 2), 1e-4, False),
    "linear-ek0q1-fixed": ("linear", "EK0", 1, "dynamic", 1.0, False, 2.0 ** -3, lambda t: [t[0], t[2] + 0.03, t[2] + 0.09, t[5], t[-1]],
                           (0, 1), 1e-4, False),
}


def gpu_like_case(name, N=2, seed=50):
    """The problem `name` of the GPU tests on oracle solves of N perturbed trajectories, in the layout of the cases above."""
    field, kind, order, diffusion, t1, adaptive, dt, times, comps, r, per_traj = GPU_PROBLEMS[name]
    vf = orc.vector_field(field)
    alg = (orc.EK1 if kind == "EK1" else orc.EK0)(order=order, diffusionmodel=diffusion, smooth=False)
    u0s = orc.ensemble_u0(vf.u0, N, 1e-2)
    r = np.broadcast_to(np.asarray(r, float), (len(comps),)).copy()
    if adaptive:
        mean, cov, diff, T, ns = adaptive_records(vf, alg, u0s, (0.0, t1), dt=dt)
        tau = np.asarray(times(T[: ns[0], 0]), float)
    else:
        mean, cov, diff, T = dr.oracle_records(vf, alg, u0s, np.arange(int(round(t1 / dt)) + 1) * dt)
        ns, tau = None, np.asarray(times(T), float)
    y = observations(mean, T, ns, tau, comps, r, per_traj, seed)
    return dict(mean=mean, cov=cov, diff=diff, t=T, nsaved=ns, d=vf.d, q=order, times=tau, comps=list(comps), y=y, r=r)
