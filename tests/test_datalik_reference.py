"""The reference of the data log-likelihood tests (tests/_datalik_reference.py) is the right quantity, shown without its recursion:
(a) the Gaussian log-density of the observed entries of the dense joint of all states, built from the smoothed marginals and the
cross-covariances Cov(x_k, x_{k+1}) = G_k Sigma^s_{k+1} in un-preconditioned coordinates; (b) one observation at the last save
against the filter record alone; (c) additivity when one component's noise grows; (d) the float64 numpy evaluation calibrates the
tolerance the kernel is held to."""
import math

import numpy as np

import _datalik_reference as dr
from _datalik_reference import orc

LD = np.longdouble


def inv_ld(Mx):
    """Gauss-Jordan inverse with partial pivoting in longdouble."""
    n = Mx.shape[0]
    a = np.concatenate([Mx.astype(LD), np.eye(n, dtype=LD)], axis=1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(a[k:, k])))
        a[[k, p]] = a[[p, k]]
        a[k] = a[k] / a[k, k]
        for i in range(n):
            if i != k:
                a[i] = a[i] - a[i, k] * a[k]
    return a[:, n:]


def chol_ld(Mx):
    n = Mx.shape[0]
    L = np.zeros((n, n), LD)
    for j in range(n):
        s = Mx[j, j] - (L[j, :j] * L[j, :j]).sum()
        assert s > 0
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, n):
            L[i, j] = (Mx[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return L


def gauss_logpdf(y, m, C):
    L = chol_ld(C)
    w = np.zeros(len(y), LD)
    for i in range(len(y)):
        w[i] = (y[i] - m[i] - (L[i, :i] * w[:i]).sum()) / L[i, i]
    return -((w * w).sum() + 2 * np.log(np.diag(L)).sum() + len(y) * LD(dr.LOG_2PI)) / 2, (w * w).sum()


def dense_joint(mean, cov_tril, diff, t, d, q):
    """Mean [n D] and covariance [n D, n D] of all states of one trajectory under the Gauss-Markov posterior, in longdouble and in
    un-preconditioned coordinates: A(h) = P^-1 A P, Q(h) = P^-1 Q P^-1."""
    n, D = mean.shape[0], d * (q + 1)
    A, Q = dr.prior(d, q, LD)
    m = [mean[k, :, 0].astype(LD) for k in range(n)]
    S = [dr.unpack(cov_tril[k][:, :1], D, LD)[0] for k in range(n)]
    G, ms, Ps = [None] * (n - 1), list(m), list(S)
    for k in range(n - 2, -1, -1):
        h = LD(t[k + 1] - t[k])
        P = dr.precond(h, d, q, LD)
        Ah = A * P[None, :] / P[:, None]
        Qh = Q / P[:, None] / P[None, :] * LD(diff[k + 1, 0])
        B = Ah @ S[k] @ Ah.T + Qh
        G[k] = S[k] @ Ah.T @ inv_ld(B)
        ms[k] = m[k] + G[k] @ (ms[k + 1] - Ah @ m[k])
        Ps[k] = S[k] + G[k] @ (Ps[k + 1] - B) @ G[k].T
    C = np.zeros((n * D, n * D), LD)
    for l in range(n):
        blk = Ps[l]
        C[l * D:(l + 1) * D, l * D:(l + 1) * D] = blk
        for k in range(l - 1, -1, -1):
            blk = G[k] @ blk
            C[k * D:(k + 1) * D, l * D:(l + 1) * D] = blk
            C[l * D:(l + 1) * D, k * D:(k + 1) * D] = blk.T
    return np.concatenate(ms), C


def _one(field, alg, tgrid, seed):
    vf = field if not isinstance(field, str) else orc.vector_field(field)
    return (vf,) + dr.oracle_records(vf, alg, [vf.u0], tgrid)


def _dense_check(vf, mean, cov, diff, t, q, saves, comps, r, seed):
    d, D = vf.d, vf.d * (q + 1)
    y = dr._observations(mean, saves, comps, np.broadcast_to(r, (len(comps),)), False, seed)
    got = dr.evaluate(mean, cov, diff, t, d, q, saves, comps, y, r)
    mj, Cj = dense_joint(mean, cov, diff, t, d, q)
    idx = [k * D + c for k in saves for c in comps]
    R = np.diag(np.tile(np.broadcast_to(np.asarray(r, float), (len(comps),)), len(saves)).astype(LD))
    want, want_q = gauss_logpdf(y.reshape(-1).astype(LD), mj[idx], Cj[np.ix_(idx, idx)] + R)
    rel = abs(got["loglik"][0] - want) / abs(want)
    print(f"{vf.name} q={q} saves={list(saves)} comps={list(comps)}: loglik {float(want):.12g}, relative difference {float(rel):.3g}")
    assert rel <= 1e-12
    return got, want_q


def test_dense_joint_linear_d1_ek0_q2():
    vf, mean, cov, diff, t = _one(dr._linear_field(1), orc.EK0(order=2), np.arange(6) * 0.2, 0)
    _dense_check(vf, mean, cov, diff, t, 2, range(6), (0,), 1e-3, 11)
    _dense_check(vf, mean, cov, diff, t, 2, (1, 4), (0,), 1e-2, 12)


def test_dense_joint_fhn_ek1_q1():
    vf, mean, cov, diff, t = _one("fhn", orc.EK1(order=1), np.arange(5) * 0.25, 0)
    _dense_check(vf, mean, cov, diff, t, 1, range(5), (0, 1), (1e-3, 2e-3), 13)
    _dense_check(vf, mean, cov, diff, t, 1, (0, 2, 3), (1,), 1e-2, 14)
    # a fixed-diffusion solve after its rescale
    vf, mean, cov, diff, t = _one("fhn", orc.EK1(order=1, diffusionmodel="fixed"), np.arange(5) * 0.25, 0)
    _dense_check(vf, mean, cov, diff, t, 1, (1, 2, 4), (0, 1), 1e-3, 15)


def test_one_observation_at_the_last_save_needs_the_filter_record_alone():
    c = dr.cases()["lorenz-ek1q5-map-N65-last"]
    ref = dr.run_reference(c)
    D, n = c["d"] * (c["q"] + 1), c["mean"].shape[0]
    for i in (0, 17, 64):
        S = dr.unpack(c["cov"][n - 1][:, i:i + 1], D, LD)[0][np.ix_(c["comps"], c["comps"])] + np.diag(c["r"]).astype(LD)
        want, want_q = gauss_logpdf(c["y"][i, 0].astype(LD), c["mean"][n - 1, c["comps"], i].astype(LD), S)
        assert abs(ref["loglik"][i] - want) <= 1e-15 * abs(want) and abs(ref["mahalanobis"][i] - want_q) <= 1e-15 * abs(want_q)


def test_additivity_as_one_components_noise_grows():
    c = dr.cases()["fhn-ek1q1-N130-4th-pertraj"]
    M = len(c["saves"])
    both = dr.evaluate(c["mean"], c["cov"], c["diff"], c["t"], c["d"], c["q"], c["saves"], (0, 1), c["y"], (c["r"][0], 1e12))
    only = dr.evaluate(c["mean"], c["cov"], c["diff"], c["t"], c["d"], c["q"], c["saves"], (0,), c["y"][:, :, :1], c["r"][:1])
    bound = dr.unit_bound(c["mean"], c["cov"], c["diff"], c["t"], c["d"], c["q"], c["saves"], (0,), c["y"][:, :, :1], c["r"][:1])
    flat = -M * (math.log(1e12) + math.log(2 * math.pi)) / 2                      # M times log N(v; 0, 1e12) at v^2 / r -> 0
    diff = np.abs((both["loglik"] - only["loglik"]).astype(float) - flat)
    v2 = (c["y"][:, :, 1] ** 2).sum(axis=1).max()
    print(f"additivity: worst |l(both) - l(first) - M log N(0; r)| = {diff.max():.3g}; coupling v^2 / r <= {v2 / 1e12:.3g}; "
          f"unit bound {bound['loglik'].max():.3g}")
    assert np.all(diff <= 4 * v2 / 1e12 + 1e-10)  # (log r itself is rounded at 28 u ~ 3e-15 per observation)
    assert np.all(np.abs((both["mahalanobis"] - only["mahalanobis"]).astype(float)) <= 4 * v2 / 1e12 + dr.DEVICE_FACTOR * bound["mahalanobis"])


def test_float64_numpy_evaluation_calibrates_the_tolerance():
    """The numpy float64 evaluation of the definition against the longdouble reference on every input of the emulation tests --
    the GPU tests run the same problems, orders, grids and observation patterns --, in units of `unit_bound`: the measured
    constant C_NUMPY is not exceeded (the device gets 16 times it)."""
    worst = 0.0
    for name, c in dr.cases().items():
        ref, f64 = dr.run_reference(c), dr.run_reference(c, np.float64)
        r = dr.ratios(f64, ref, dr.case_bound(c))
        print(name, {k: f"{v:.3g}" for k, v in r.items()})
        worst = max(worst, *r.values())
    print(f"numpy float64 / unit bound, worst: {worst:.3g} (C_NUMPY = {dr.C_NUMPY})")
    assert worst <= dr.C_NUMPY
    assert worst >= dr.C_NUMPY / 4  # the constant is the measured value rounded up, not a loose guess
