"""The data log-likelihood of noisy observations per trajectory in extended precision: the yardstick of the data-likelihood
tests ("exact").

The filter records (m_k, Sigma_k) of a fixed grid t_0 .. t_{n-1} and the backward transitions of the RTS smoother define a
Gauss-Markov posterior over the path.  The marginal likelihood of y_j = H x(t_{k_j}) + N(0, diag r), H the rows `comps` of E0,
under it is one backward sweep (Tronarp, Bosch, Hennig 2022, "Fenrir"; include/odefilter.h, odef_data_field):

    xi = (m_{n-1}, Sigma_{n-1});  l = 0;  q = 0
    for k = n-1 down to k_1:
      if k < n-1:  h = t_{k+1} - t_k
         h == 0: xi unchanged
         else, in the coordinates preconditioned with P(h):
            B = A Sigma_k A' + sigma2_k Q;  G = Sigma_k A' B^-1
            xi.m <- m_k + G (xi.m - A m_k);   xi.P <- Sigma_k + G (xi.P - B) G'
      if k = k_j:  v = y_j - H xi.m;  S = H xi.P H' + R
         l += -1/2 (v' S^-1 v + log det S + o log 2 pi);  q += v' S^-1 v
         K = xi.P H' S^-1;  xi.m += K v;  xi.P -= K S K'

sigma2_k is the diffusion the smoother uses for the step t_k -> t_{k+1}: `diffusion[k + 1]` in the device layout (slot s holds the
diffusion of the step that produced save s; oracle/odefilter_oracle.py:smooth_all reads sol.diffusions[k]).  B is factored
L D L' with the project's zero-pivot rule (a non-positive pivot drops its direction); a non-positive pivot of S, or a NaN in a
record the sweep reads, gives NaN for that trajectory.  A, Q are the float64 constants the library holds (part of the input).

Records are in the device layout: mean [n_save, D, N], cov_tril [n_save, TRI, N], diffusion [n_save, N], t [n_save];
saves [M], comps [o], y [M, o] (shared) or [N, M, o], r [o].  `evaluate(..., dtype=np.longdouble)` is the reference; the same
function with dtype=np.float64 is the plain numpy float64 evaluation whose own error against the reference calibrates the
tolerance (C_NUMPY below).  Shares no code with the library's host layer."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import odefilter_oracle as orc  # noqa: E402

U = 2.0 ** -53
KEYS = ("loglik", "mahalanobis")
LOG_2PI = "1.8378770664093454835606594728112352797227949472755668"

# Worst error / unit bound of the numpy FLOAT64 evaluation of the definition against the longdouble reference over the inputs of
# tests/test_datalik_emul.py and tests/test_gpu_datalik.py (test_float64_numpy_evaluation_calibrates_the_tolerance measures it
# again and asserts that it is not exceeded).  The device is given EXACT_FACTOR = 16 times that (tests/_parity.py): the margin a
# different but equally valid order of the same float64 operations gets.
C_NUMPY = 0.03
DEVICE_FACTOR = 16.0


def prior(d, q, dtype):
    """A and Q of the preconditioned IBM prior (D x D), the float64 constants the library builds, cast to `dtype`."""
    A, _ = orc.ibm(d, q)
    Qt = np.zeros((q + 1, q + 1))
    for r in range(q + 1):
        for c in range(q + 1):
            Qt[r, c] = 1.0 / ((2 * q + 1 - r - c) * math.factorial(q - r) * math.factorial(q - c))
    return A.astype(dtype), np.kron(Qt, np.eye(d)).astype(dtype)


def precond(h, d, q, dtype):
    """diag of P(h) = h^(j - q - 1/2) per derivative block, [..., D]."""
    h = np.asarray(h, dtype)
    val = h ** (dtype(-q) - dtype(1) / dtype(2))
    out = []
    for _ in range(q + 1):
        out += [val] * d
        val = val * h
    return np.stack(out, axis=-1)


def unpack(tril, D, dtype):
    """[TRI, N] packed lower triangle -> [N, D, D] symmetric."""
    N = tril.shape[-1]
    out = np.zeros((N, D, D), dtype)
    k = 0
    for i in range(D):
        for j in range(i + 1):
            out[:, i, j] = out[:, j, i] = tril[k]
            k += 1
    return out


def ldl(B, drop):
    """Batched B = L D L' ([N, n, n], lower triangle read): unit lower L, 1 / D_k.  drop=True: a non-positive pivot drops its
    direction (reciprocal 0, column of L zeroed); drop=False: it gives `bad`.  Returns (L, dinv, D, bad [N])."""
    B = B.copy()
    N, n, _ = B.shape
    dt = B.dtype.type
    L = np.zeros_like(B)
    dinv = np.zeros((N, n), B.dtype)
    piv_all = np.zeros((N, n), B.dtype)
    bad = np.zeros(N, bool)
    for k in range(n):
        piv = B[:, k, k]
        pos = piv > 0
        bad |= ~pos
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = np.where(pos, dt(1) / np.where(pos, piv, dt(1)), dt(0))
        dinv[:, k] = inv
        piv_all[:, k] = piv
        L[:, k, k] = dt(1)
        if k + 1 < n:
            v = B[:, k + 1:, k].copy()
            l = v * inv[:, None]
            L[:, k + 1:, k] = l
            B[:, k + 1:, k + 1:] -= l[:, :, None] * v[:, None, :]
    return L, dinv, piv_all, (np.zeros(N, bool) if drop else bad)


def solve_lower_unit(L, Y):
    """L^-1 Y, L [N, n, n] unit lower, Y [N, n, m]."""
    Y = Y.copy()
    n = L.shape[1]
    for k in range(n):
        if k:
            Y[:, k, :] -= np.einsum("nc,ncm->nm", L[:, k, :k], Y[:, :k, :])
    return Y


def solve_upper_unit(L, Y):
    """L^-T Y."""
    Y = Y.copy()
    n = L.shape[1]
    for k in range(n - 2, -1, -1):
        Y[:, k, :] -= np.einsum("nc,ncm->nm", L[:, k + 1:, k], Y[:, k + 1:, :])
    return Y


def pinv_apply(L, dinv, Y):
    """B^+ Y from the factorisation."""
    return solve_upper_unit(L, solve_lower_unit(L, Y) * dinv[:, :, None])


def _records(mean, cov_tril, diffusion):
    mean, cov_tril, diffusion = np.asarray(mean), np.asarray(cov_tril), np.asarray(diffusion)
    if mean.ndim == 2:
        mean, cov_tril, diffusion = mean[:, :, None], cov_tril[:, :, None], diffusion.reshape(-1, 1)
    return mean, cov_tril, diffusion


def _values(y, N, M, o):
    y = np.asarray(y)
    if y.ndim == 2:
        y = np.broadcast_to(y[None], (N, M, o))
    assert y.shape == (N, M, o), y.shape
    return y


def sweep(mean, cov_tril, diffusion, t, d, q, saves, comps, y, r, dtype=np.longdouble, on_step=None, on_obs=None):
    """The definition.  `on_step(k, B, X)` (preconditioned) and `on_obs(j, v, S, xm, xP)` see the intermediate values."""
    mean, cov_tril, diffusion = _records(mean, cov_tril, diffusion)
    n, D, N = mean.shape
    assert D == d * (q + 1)
    saves, comps = [int(s) for s in saves], [int(c) for c in comps]
    M, o = len(saves), len(comps)
    y = _values(y, N, M, o)
    r = np.broadcast_to(np.asarray(r, float), (o,)).astype(dtype)
    t = np.asarray(t, np.float64)
    A, Q = prior(d, q, dtype)
    dt = np.dtype(dtype).type
    bad = np.isnan(mean[n - 1]).any(axis=0) | np.isnan(cov_tril[n - 1]).any(axis=0)
    xm = mean[n - 1].T.astype(dtype)             # [N, D]
    xP = unpack(cov_tril[n - 1], D, dtype)       # [N, D, D]
    ll = np.zeros(N, dtype)
    qq = np.zeros(N, dtype)
    logdet = np.zeros(N, dtype)
    j = M - 1
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for k in range(n - 1, saves[0] - 1, -1):
            h = (t[k + 1] - t[k]) if k < n - 1 else 0.0  # (the float64 difference is the input the device sees)
            if h != 0.0:
                bad |= np.isnan(mean[k]).any(axis=0) | np.isnan(cov_tril[k]).any(axis=0) | np.isnan(diffusion[k + 1])
                P = precond(h, d, q, dtype)
                Pi = dt(1) / P
                X = unpack(cov_tril[k], D, dtype) * P[:, None] * P[None, :]
                mt = mean[k].T.astype(dtype) * P
                s2 = diffusion[k + 1].astype(dtype)
                B = A @ X @ A.T + s2[:, None, None] * Q
                B = (B + B.transpose(0, 2, 1)) / dt(2)
                if on_step:
                    on_step(k, B, X)
                L, dinv, _, _ = ldl(B, drop=True)
                Gt = pinv_apply(L, dinv, A @ X)          # G' = B^+ A X
                G = Gt.transpose(0, 2, 1)
                ms = xm * P
                Ps = xP * P[:, None] * P[None, :]
                xm = (mt + np.einsum("nij,nj->ni", G, ms - mt @ A.T)) * Pi
                xP = (X + G @ (Ps - B) @ Gt) * Pi[:, None] * Pi[None, :]
                xP = (xP + xP.transpose(0, 2, 1)) / dt(2)
            if j >= 0 and k == saves[j]:
                yj = y[:, j, :].astype(dtype)
                bad |= np.isnan(y[:, j, :]).any(axis=1)
                v = yj - xm[:, comps]
                S = xP[:, comps][:, :, comps] + np.diag(r)
                if on_obs:
                    on_obs(j, v, S, xm, xP)
                L, dinv, piv, sbad = ldl(S, drop=False)
                bad |= sbad
                w = solve_lower_unit(L, v[:, :, None])[:, :, 0]
                qj = (w * w * dinv).sum(axis=1)
                qq = qq + qj
                logdet = logdet + np.log(np.where(piv > 0, piv, dt(1))).sum(axis=1)
                HP = xP[:, comps, :]                       # [N, o, D]
                Kt = pinv_apply(L, dinv, HP)               # K' = S^-1 H P
                xm = xm + np.einsum("nod,no->nd", Kt, v)
                xP = xP - HP.transpose(0, 2, 1) @ Kt
                xP = (xP + xP.transpose(0, 2, 1)) / dt(2)
                j -= 1
    ll = -(qq + logdet + dt(M * o) * dtype(LOG_2PI)) / dt(2)
    nan = dt(np.nan)
    return {"loglik": np.where(bad, nan, ll), "mahalanobis": np.where(bad, nan, qq)}


def evaluate(mean, cov_tril, diffusion, t, d, q, saves, comps, y, r, dtype=np.longdouble):
    """dict with loglik, mahalanobis [N] in `dtype`."""
    return sweep(mean, cov_tril, diffusion, t, d, q, saves, comps, y, r, dtype)


def _cond(Mx):
    """Ratio of the extreme positive eigenvalues of the symmetric matrices [N, n, n] (1 where none is positive or finite)."""
    Mx = np.where(np.isfinite(Mx), Mx, 0.0)
    w = np.linalg.eigvalsh(Mx)
    big = w.max(axis=-1)
    pos = w > 1e-13 * np.maximum(big, 1e-300)[:, None]
    small = np.where(pos, w, np.inf).min(axis=-1)
    c = big / small
    return np.where(np.isfinite(c) & (c >= 1.0), c, 1.0)


def unit_bound(mean, cov_tril, diffusion, t, d, q, saves, comps, y, r):
    """The unit of the tolerance per trajectory (float64 [N] for each key); the allowed error is c times it.  With u = 2^-53:

    every RTS step solves with B_k, which loses a factor cond(B_k) of the digits of xi; over the steps swept so far that is
        acc = sum_k D cond(B_k)          (+ o cond(S_j) for every measurement update already made)
    At observation j the innovation v = y - H xi.m is rounded against |y| + |H xi.m| and inherits the sweep's error,
        delta_v = u (1 + acc) (|y| + |H xi.m|),
    and S inherits it relative to itself, eps_S = u (1 + acc).  Then
        |delta (v' S^-1 v)|  <=  2 |v|' |S^-1| delta_v + (o u + eps_S) cond(S) v' S^-1 v
        |delta log det S|    <=  o eps_S cond(S) + u |log det S|
    and the sums over the M observations add (M + 2) u times their value.  loglik takes half of both, mahalanobis the first."""
    D = d * (q + 1)
    o = len(comps)
    st = {"acc": None, "bq": None, "bl": None}

    def on_step(k, B, X):
        c = D * _cond(B.astype(float))
        st["acc"] = c if st["acc"] is None else st["acc"] + c

    def on_obs(j, v, S, xm, xP):
        N = v.shape[0]
        acc = np.zeros(N) if st["acc"] is None else st["acc"]
        Sf = np.where(np.isfinite(S.astype(float)), S.astype(float), 0.0)
        vf = np.nan_to_num(np.abs(v.astype(float)))
        yj = np.nan_to_num(np.abs(_values(y, N, len(saves), o)[:, j, :].astype(float)))
        hm = np.nan_to_num(np.abs(xm.astype(float)[:, list(comps)]))
        cS = _cond(Sf)
        Sinv = np.abs(np.linalg.pinv(Sf))
        dv = U * (1.0 + acc)[:, None] * (yj + hm)
        qj = np.einsum("ni,nij,nj->n", vf, Sinv, vf)
        eps = U * (1.0 + acc)
        bq = 2.0 * np.einsum("ni,nij,nj->n", vf, Sinv, dv) + (o * U + eps) * cS * qj
        sign, ld = np.linalg.slogdet(np.where(np.eye(o, dtype=bool), np.maximum(Sf, 1e-300), Sf))
        bl = o * eps * cS + U * np.abs(np.nan_to_num(ld))
        st["bq"] = bq if st["bq"] is None else st["bq"] + bq
        st["bl"] = bl if st["bl"] is None else st["bl"] + bl
        st["acc"] = acc + o * cS

    with np.errstate(all="ignore"):
        ref = sweep(mean, cov_tril, diffusion, t, d, q, saves, comps, y, r, np.float64, on_step, on_obs)
    M = len(saves)
    ll = np.nan_to_num(np.abs(ref["loglik"]))
    qq = np.nan_to_num(np.abs(ref["mahalanobis"]))
    return {"loglik": 0.5 * (st["bq"] + st["bl"]) + (M + 2) * U * ll, "mahalanobis": st["bq"] + (M + 2) * U * qq}


def ratios(got, ref, bounds):
    """Worst |got - ref| / unit bound per key over the trajectories whose reference is finite; asserts that NaN meets NaN."""
    out = {}
    for k in KEYS:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        gn, rn = np.isnan(g.astype(float)), np.isnan(r.astype(float))
        assert np.array_equal(gn, rn), (k, np.flatnonzero(gn != rn))
        fin = ~rn
        err = np.abs(g[fin].astype(np.longdouble) - r[fin].astype(np.longdouble)).astype(float)
        b = bounds[k][fin]
        assert np.all(b[err > 0] > 0), (k, "an error where the bound is zero")
        out[k] = float((err[err > 0] / b[err > 0]).max()) if np.any(err > 0) else 0.0
    return out


def check(got, ref, bounds, factor=DEVICE_FACTOR, label=""):
    """Asserts |got - ref| <= factor C_NUMPY unit bound for both quantities; returns the ratios error / unit bound."""
    rt = ratios(got, ref, bounds)
    for k in KEYS:
        assert rt[k] <= factor * C_NUMPY, (label, k, rt[k], factor * C_NUMPY)
    return rt


def oracle_records(vf, alg, u0s, tgrid, ps=None, repeat_at=()):
    """Device-layout filter records of oracle solves of the trajectories u0s [N, d] on a fixed grid: (mean [n, D, N], cov_tril
    [n, TRI, N], diffusion [n, N], t [n]).  `ps`: per-trajectory parameters.  `repeat_at`: record indices after which the record is
    planted again at the unchanged time (a grid with h = 0)."""
    sols = [orc.solve(vf, alg, u0=u0, p=None if ps is None else ps[i], tgrid=tgrid) for i, u0 in enumerate(u0s)]
    d, q = sols[0].d, sols[0].q
    D = d * (q + 1)
    il = np.tril_indices(D)
    cols = []
    for s in sols:
        mu, cov, t = list(s.means(False)), list(s.covs(False)), list(s.t)
        df = [0.0] + list(s.diffusions)  # slot k + 1: the step k -> k + 1
        for k in sorted(repeat_at, reverse=True):
            mu.insert(k + 1, mu[k]); cov.insert(k + 1, cov[k]); t.insert(k + 1, t[k]); df.insert(k + 1, df[k])
        cols.append((np.array(mu), np.array(cov)[:, il[0], il[1]], np.array(df), np.array(t)))
    mean = np.ascontiguousarray(np.stack([c[0] for c in cols], axis=-1))
    covt = np.ascontiguousarray(np.stack([c[1] for c in cols], axis=-1))
    diff = np.ascontiguousarray(np.stack([c[2] for c in cols], axis=-1))
    return mean, covt, diff, cols[0][3]


# ---- the inputs of tests/test_datalik_emul.py (and of the calibration in tests/test_datalik_reference.py) -------------------------

def _linear_field(d):
    """u' = p u on d components (oracle `linear`, any d)."""
    base = orc.vector_field("linear")
    p = np.array([1.1, -0.5, -0.9, 0.4][:d]) if d > 1 else np.array([-0.7])
    u0 = np.array([0.1, 1.0, 0.6, -0.8][:d]) if d > 1 else np.array([1.0])
    return orc.VectorField(f"linear{d}", base.rhs_id, d, d, base.f, base.jac, u0, p, (0.0, 1.0))


def _observations(mean, saves, comps, r, per_traj, seed):
    """y = H m_k of the records (trajectory 0 when shared) plus seeded N(0, r) noise: [M, o] or [N, M, o]."""
    rng = np.random.default_rng(seed)
    hm = np.nan_to_num(mean[np.asarray(saves)][:, np.asarray(comps), :])          # [M, o, N]
    noise = rng.standard_normal(hm.shape) * np.sqrt(np.asarray(r, float))[None, :, None]
    y = (hm + noise).transpose(2, 0, 1)
    return np.ascontiguousarray(y) if per_traj else np.ascontiguousarray(y[0])


def _case(field, alg, N, tgrid, saves, comps, r, per_traj, seed, distinct=5, scale=1e-2, repeat_at=()):
    """Oracle records of `distinct` perturbed initial values, repeated to N trajectories whose means then differ per lane by a
    relative 1e-3 (any records are a valid input of the pass; every lane has its own numbers)."""
    vf = field if not isinstance(field, str) else orc.vector_field(field)
    nd = min(N, distinct)
    u0s = orc.ensemble_u0(vf.u0, nd, scale)
    mean, cov, diff, t = oracle_records(vf, alg, u0s, tgrid, repeat_at=repeat_at)
    reps = -(-N // nd)
    mean, cov, diff = (np.ascontiguousarray(np.tile(a, reps)[..., :N]) for a in (mean, cov, diff))
    rng = np.random.default_rng(seed + 1)
    mean = mean * (1.0 + 1e-3 * rng.standard_normal((1, 1, N)))
    n = mean.shape[0]
    saves = [s if s >= 0 else n + s for s in saves]
    r = np.broadcast_to(np.asarray(r, float), (len(comps),)).copy()
    y = _observations(mean, saves, comps, r, per_traj, seed)
    return dict(mean=mean, cov=cov, diff=diff, t=t, d=vf.d, q=alg.order, saves=saves, comps=list(comps), y=y, r=r)


def _build_cases():
    g = lambda n, h: np.arange(n) * h  # noqa: E731
    c = {}
    c["lin1-ek0q1-N1-all"] = _case(_linear_field(1), orc.EK0(order=1), 1, g(5, 0.125), range(5), (0,), 1e-4, False, 1)
    c["lin1-ek1q4-N65-save0"] = _case(_linear_field(1), orc.EK1(order=4), 65, g(9, 0.125), (0,), (0,), 1e-3, False, 2)
    c["fhn-ek1q1-N130-4th-pertraj"] = _case("fhn", orc.EK1(order=1), 130, g(17, 0.0625), range(0, 17, 4), (0, 1), (1e-3, 4e-3), True, 3)
    c["lv-ek0q3-fixed-N65-interior"] = _case("lotka_volterra", orc.EK0(order=3, diffusionmodel="fixed"), 65, g(12, 0.0625), (5,), (1,),
                                             1e-2, False, 4)
    c["lorenz-ek1q3-N130-c02-4th"] = _case("lorenz63", orc.EK1(order=3), 130, g(33, 2.0 ** -6), range(0, 33, 4), (0, 2), 1e-2, False, 5)
    c["lorenz-ek1q5-map-N65-last"] = _case("lorenz63", orc.EK1(order=5, diffusionmodel="fixedMAP"), 65, g(17, 2.0 ** -5), (-1,),
                                           (0, 1, 2), 1e-2, True, 6)
    c["lin4-ek0q4-N65-all"] = _case(_linear_field(4), orc.EK0(order=4), 65, g(7, 0.125), range(7), (0, 1, 2, 3), 1e-3, False, 7)
    c["lin2-ek0q3-N130-all-pertraj"] = _case("linear", orc.EK0(order=3), 130, g(10, 0.125), range(10), (0, 1), 1e-4, True, 8)
    c["fhn-ek1q3-N65-4th"] = _case("fhn", orc.EK1(order=3), 65, g(17, 0.0625), range(0, 17, 4), (1,), 1e-3, False, 9)
    # a grid with a repeated time: records 3 and 7 planted again (h = 0), the copies observed too
    c["fhn-ek1q1-N65-repeat"] = _case("fhn", orc.EK1(order=1), 65, g(15, 0.0625), (0, 3, 4, 8, 9, 16), (0, 1), 1e-3, False, 10,
                                      repeat_at=(3, 7))
    return c


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _build_cases()
    return _CASES


def run_reference(c, dtype=np.longdouble):
    return evaluate(c["mean"], c["cov"], c["diff"], c["t"], c["d"], c["q"], c["saves"], c["comps"], c["y"], c["r"], dtype)


def case_bound(c):
    return unit_bound(c["mean"], c["cov"], c["diff"], c["t"], c["d"], c["q"], c["saves"], c["comps"], c["y"], c["r"])
