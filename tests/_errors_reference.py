"""The per-trajectory solution errors in extended precision: the yardstick of the error tests ("exact").

For trajectory i over its own saves k, e_k = u_k - u*_k (u_k rows 0..d-1 of the mean, Sigma_k the d x d solution block):
    final = mean_a |e_{n-1,a}|,  l2 = sqrt(mean_{k,a} e_{k,a}^2),  linf = max_{k,a} |e_{k,a}|
are DiffEqBase's `calculate_solution_errors!` (third party, restated: `:final`, `:l2`, `:l∞` of timeseries_errors);
    chi2 = mean_k e_k' Sigma_k^+ e_k / d
is this project's calibration statistic, over the saves whose block is not exactly zero (NaN when none is left), the block
factored Sigma = L D L' with the project's zero-pivot rule: a non-positive pivot drops its direction.  Records are in the device
layout -- mean [n_save, D, N], cov_tril [n_save, TRI, N], truth [n_save, d, N] --; an adaptive solve brings tsave [n_save, N]
and nsaved [N]: saves k >= nsaved and zero-length repeats (t_k == t_{k-1}) are not saves of the solution.

`evaluate(..., dtype=np.longdouble)` is the reference; the same function with dtype=np.float64 is the plain numpy float64
evaluation whose own error against the reference calibrates the tolerances (C_NUMPY below).  `oracle_records` builds records from
oracle/odefilter_oracle.py solutions.  Shares no code with the library's host layer."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import odefilter_oracle as orc  # noqa: E402

U = 2.0 ** -53
KEYS = ("final", "l2", "linf", "chi2")

# Worst error / unit bound of the numpy FLOAT64 evaluation of these definitions against the longdouble reference over the inputs of
# tests/test_errors_emul.py (test_float64_numpy_evaluation_calibrates_the_tolerances measures them again and asserts that they are
# not exceeded).  The device is given 16 times that -- the margin `check_against_exact` uses, for the same reason: a different
# but equally valid order of the same float64 operations.
C_NUMPY = {"final": 0.32, "l2": 0.049, "linf": 0.14, "chi2": 0.44}
DEVICE_FACTOR = 16.0


def tri(d):
    return d * (d + 1) // 2


def used_mask(n_save, N, tsave=None, nsaved=None):
    """[n_save, N] bool: the saves of the solution."""
    used = np.ones((n_save, N), bool)
    if nsaved is not None:
        used &= np.arange(n_save)[:, None] < np.asarray(nsaved)[None, :]
    if tsave is not None:
        t = np.asarray(tsave).reshape(n_save, N)
        used[1:] &= t[1:] != t[:-1]
    return used


def _quad(S, e, dtype):
    """e' Sigma^+ e by elimination with the zero-pivot rule, vectorised over the leading axes.  S [..., d, d] (lower triangle
    read), e [..., d]; both are overwritten."""
    d = e.shape[-1]
    q = np.zeros(e.shape[:-1], dtype)
    one = dtype(1)
    for k in range(d):
        piv = S[..., k, k]
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = np.where(piv <= 0, dtype(0), one / piv)
        y = e[..., k]
        q = q + y * y * inv
        for i in range(k + 1, d):
            l = S[..., i, k] * inv
            e[..., i] = e[..., i] - l * y
            for j in range(k + 1, i + 1):
                S[..., i, j] = S[..., i, j] - l * S[..., j, k]
    return q


def evaluate(mean, cov_tril, d, truth, tsave=None, nsaved=None, dtype=np.longdouble):
    """dict with final, l2, linf, chi2 [N] in `dtype` and nused [N] int64."""
    mean, cov_tril = np.asarray(mean), np.asarray(cov_tril)
    n_save, _, N = mean.shape
    used = used_mask(n_save, N, tsave, nsaved)
    nused = used.sum(axis=0).astype(np.int64)
    e = mean[:, :d, :].astype(dtype) - np.asarray(truth).astype(dtype)  # [n_save, d, N]
    ae = np.abs(e)
    nan = dtype(np.nan)
    last = np.where(nused > 0, n_save - 1 - np.argmax(used[::-1], axis=0), 0)
    final = np.where(nused > 0, ae[last, :, np.arange(N)].sum(axis=1) / d, nan)
    um = used[:, None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        l2 = np.sqrt(np.where(um, e * e, dtype(0)).sum(axis=(0, 1)) / (nused.astype(dtype) * d))
        linf = np.where(nused > 0, np.where(um, ae, dtype(0)).max(axis=(0, 1)), nan)  # (np.max propagates NaN)
    blk = cov_tril[:, : tri(d), :]
    nonzero = used & np.any(blk != 0, axis=1)
    S = np.zeros((n_save, N, d, d), dtype)
    for a in range(d):
        for b in range(a + 1):
            S[:, :, a, b] = blk[:, a * (a + 1) // 2 + b, :]
    with np.errstate(invalid="ignore", over="ignore"):
        qk = _quad(S, np.ascontiguousarray(e.transpose(0, 2, 1)), dtype)  # [n_save, N]
    nchi = nonzero.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        chi2 = np.where(nonzero, qk, dtype(0)).sum(axis=0) / nchi.astype(dtype) / d
    # a NaN at a save that is left out must not leak through the zero of np.where; one at a save that counts must stay
    return {"final": final.astype(dtype), "l2": l2, "linf": linf, "chi2": chi2, "nused": nused}


def unit_bounds(mean, cov_tril, d, truth, ref, tsave=None, nsaved=None):
    """The unit of each tolerance (float64 [N]); the allowed error is c times it.  With m = |u| + |u*| per entry (what a
    difference u - u* that cancels is rounded against) and u = 2^-53:
        final  u mean_a m_{n-1,a}
        linf   u max_{k,a} m_{k,a}
        l2     u (sqrt(mean_{k,a} m^2) + (n d + 2) l2)            [Cauchy-Schwarz on sum |e| delta, plus the summation]
        chi2   mean_k (2 |e_k|' |Sigma_k^+| delta_k + d cond(Sigma_k) u chi_k) / d + (n + 2) u chi2,  delta = u m,
    cond the ratio of the extreme positive eigenvalues of the block."""
    mean, cov_tril = np.asarray(mean, float), np.asarray(cov_tril, float)
    n_save, _, N = mean.shape
    used = used_mask(n_save, N, tsave, nsaved)
    nused = used.sum(axis=0)
    tr = np.asarray(truth).astype(float)
    m = np.abs(mean[:, :d, :]) + np.abs(tr)
    e = np.abs(mean[:, :d, :] - tr)
    um = used[:, None, :]
    last = np.where(nused > 0, n_save - 1 - np.argmax(used[::-1], axis=0), 0)
    b_final = U * m[last, :, np.arange(N)].sum(axis=1) / d
    b_linf = U * np.where(um, m, 0.0).max(axis=(0, 1))
    nd = np.maximum(nused, 1) * d
    b_l2 = U * (np.sqrt(np.where(um, m * m, 0.0).sum(axis=(0, 1)) / nd) + (nd + 2) * np.nan_to_num(ref["l2"].astype(float)))
    blk = cov_tril[:, : tri(d), :]
    nonzero = used & np.any(blk != 0, axis=1)
    S = np.zeros((n_save, N, d, d))
    for a in range(d):
        for b in range(a + 1):
            S[:, :, a, b] = S[:, :, b, a] = blk[:, a * (a + 1) // 2 + b, :]
    S = np.where(np.isfinite(S), S, 0.0)
    w, V = np.linalg.eigh(S)
    big = w.max(axis=-1, keepdims=True)
    pos = w > 1e-13 * np.maximum(big, 1e-300)
    winv = np.where(pos, 1.0 / np.where(pos, w, 1.0), 0.0)
    P = np.abs(np.einsum("...ij,...j,...kj->...ik", V, winv, V))  # |Sigma^+|
    cond = big[..., 0] / np.where(pos, w, np.inf).min(axis=-1)
    ek = np.nan_to_num(e.transpose(0, 2, 1))
    dk = U * np.nan_to_num(m.transpose(0, 2, 1))
    chi_k = np.einsum("...i,...ij,...j->...", ek, P, ek)
    per = 2.0 * np.einsum("...i,...ij,...j->...", ek, P, dk) + d * np.where(np.isfinite(cond), cond, 1.0) * U * chi_k
    nchi = np.maximum(nonzero.sum(axis=0), 1)
    b_chi2 = np.where(nonzero, per, 0.0).sum(axis=0) / nchi / d + (nchi + 2) * U * np.nan_to_num(ref["chi2"].astype(float))
    return {"final": b_final, "l2": b_l2, "linf": b_linf, "chi2": b_chi2}


def ratios(got, ref, bounds):
    """Worst |got - ref| / unit bound per quantity over the trajectories whose reference is finite; asserts that NaN meets NaN and
    that NUSED agrees exactly."""
    assert np.array_equal(np.asarray(got["nused"], np.int64), ref["nused"]), (got["nused"], ref["nused"])
    out = {}
    for k in KEYS:
        g, r = np.asarray(got[k]), ref[k]
        fin = np.isfinite(r.astype(float))
        assert np.array_equal(np.isnan(g.astype(float)), np.isnan(r.astype(float))), (k, g, r)
        assert np.array_equal(g[~fin & ~np.isnan(r.astype(float))].astype(float), r[~fin & ~np.isnan(r.astype(float))].astype(float)), k
        err = np.abs(g[fin].astype(np.longdouble) - r[fin].astype(np.longdouble)).astype(float)
        b = bounds[k][fin]
        assert np.all(b[err > 0] > 0), (k, "an error where the bound is zero", err, b)
        out[k] = float((err[err > 0] / b[err > 0]).max()) if np.any(err > 0) else 0.0
    return out


def check(got, ref, bounds, factor=DEVICE_FACTOR, label=""):
    """Asserts |got - ref| <= factor C_NUMPY unit bound for the four quantities; returns the ratios error / unit bound."""
    r = ratios(got, ref, bounds)
    for k in KEYS:
        assert r[k] <= factor * C_NUMPY[k], (label, k, r[k], factor * C_NUMPY[k])
    return r


def linear_truth(u0, p, t, dtype=np.longdouble):
    """u0 [N, 2], p [2] or [N, 2], t [n_save] or [n_save, N] -> u* [n_save, 2, N] = u0 exp(p t) (test/convergence.jl:13)."""
    u0, p, t = np.asarray(u0).astype(dtype), np.asarray(p).astype(dtype), np.asarray(t).astype(dtype)
    N = u0.shape[0]
    if t.ndim == 1:
        t = np.repeat(t[:, None], N, axis=1)
    if p.ndim == 1:
        p = np.repeat(p[None, :], N, axis=0)
    return u0.T[None, :, :] * np.exp(p.T[None, :, :] * t[:, None, :])


def oracle_records(vf, alg, u0s, *, tgrid=None, adaptive=None, smoothed=False, repeat_at=()):
    """Device-layout records of oracle solves of the trajectories u0s [N, d]: (mean [n_save, D, N], cov_tril [n_save, TRI, N],
    tsave, nsaved).  Fixed grid: tsave = tgrid, nsaved None.  adaptive = dict(t1, dt0, abstol, reltol): per-trajectory records,
    zero-padded, tsave [n_save, N]; `repeat_at`: record indices after which the record is planted again at the unchanged time
    (what a rejected attempt leaves on the device)."""
    sols = []
    for u0 in u0s:
        if adaptive is None:
            sols.append(orc.solve(vf, alg, u0=u0, tgrid=tgrid))
        else:
            sols.append(orc.solve(vf, alg, u0=u0, tspan=(vf.tspan[0], adaptive["t1"]), adaptive=True, dt=adaptive["dt0"],
                                  abstol=adaptive["abstol"], reltol=adaptive["reltol"]))
    d, q = sols[0].d, sols[0].q
    D = d * (q + 1)
    il = np.tril_indices(D)
    recs = []
    for s in sols:
        mu, cov, t = s.means(smoothed), s.covs(smoothed), list(s.t)
        mu, cov = list(mu), list(cov)
        for k in sorted(repeat_at, reverse=True):
            if 0 < k < len(t):
                mu.insert(k + 1, mu[k]); cov.insert(k + 1, cov[k]); t.insert(k + 1, t[k])
        recs.append((np.array(mu), np.array(cov), np.array(t)))
    n_save = max(len(r[2]) for r in recs) + (1 if adaptive is not None else 0)  # (one unused slot past the longest)
    N = len(recs)
    mean, covt = np.zeros((n_save, D, N)), np.zeros((n_save, len(il[0]), N))
    tsave, nsaved = np.zeros((n_save, N)), np.zeros(N, np.int32)
    for i, (mu, cov, t) in enumerate(recs):
        n = len(t)
        mean[:n, :, i] = mu
        covt[:n, :, i] = cov[:, il[0], il[1]]
        tsave[:n, i] = t
        nsaved[i] = n
    if adaptive is None:
        return mean, covt, np.asarray(tgrid, float), None
    return mean, covt, tsave, nsaved
