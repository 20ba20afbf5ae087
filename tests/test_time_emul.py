"""Host build of the filter kernels around the time-dependent field RhsForced (tests/emul/emul_time.cpp: the lane kernel with
plain and lagged record stores, the row-team kernel, the adaptive kernels, the IEKS and MV twins, P.tgrid set) against the
reference for time-dependent fields (tests/_time_reference.py), with the unchanged emulated smoother on top (CPU only)."""
import ctypes as C
import functools
import glob
import os
import subprocess

import numpy as np
import pytest

import _emul as em
import _ieks_reference as ier
import _mv_reference as mvr
import _parity as P
import _time_reference as tr
import odefilter_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
MODELS = {"dynamic": 0, "fixed": 1, "fixedMAP": 2, "dynamicMV": 3, "fixedMV": 4}
# three distinct step sizes, not in order, on a grid that does not start at zero
GRID = 0.25 + np.concatenate([[0.0], np.cumsum([2.0**-6] * 5 + [2.0**-5] * 4 + [3 * 2.0**-7] * 3 + [2.0**-6] * 4 + [2.0**-5] * 3)])


def lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(HERE, "emul", "emul_time.cpp")
        out = os.path.join(HERE, "emul", "libodef_emul_time.so")
        deps = [src, os.path.join(HERE, "emul", "emul.cpp")] + glob.glob(os.path.join(em.ROOT, "odefilters.jl_amd", "csrc", "*.h"))
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            subprocess.check_call(["g++", "-O1", "-std=c++20", "-shared", "-fPIC", "-Wno-unknown-pragmas", src, "-o", out])
        _LIB = C.CDLL(out)
        _LIB.emul_precond_fill.argtypes = [C.c_int, C.c_double, C.c_double, em.dp]
    return _LIB


def emul_time(q, ek1, u0s, p, model, kernel, *, grid=None, adaptive=None, lin=None, everystep=True, smooth=True, ps=None):
    """One solve of `forced` on the emulated kernels.  grid: fixed grid; adaptive: dict(t0, t1, abstol, reltol, dt0, max_save).
    ps: parameters per trajectory [N, 3] in place of the shared p.  Returns the device layout transposed to trajectory-major,
    as _emul.emul_solve does."""
    d = 2
    u0s = np.asarray(u0s, float)
    N, D = u0s.shape[0], d * (q + 1)
    TRI = D * (D + 1) // 2
    mv = MODELS[model] >= 3
    At, Qt, QLt = em.prior_tables(q)
    u0_dev = np.ascontiguousarray(u0s.T)
    p = np.ascontiguousarray(np.asarray(p, float) if ps is None else np.asarray(ps, float).T)
    ctrl = np.array([7.0 / (10 * (q + 1)), 2.0 / (5 * (q + 1)), 0.9, 0.2, 10.0, 1.0, 1.0, 1e-4, 0.0, 1e300])
    a = em.EmulArgs()
    a.rhs, a.q, a.ek1, a.adaptive = tr.RHS_FORCED, q, int(ek1), int(adaptive is not None)
    a.N, a.u0, a.p, a.p_shared = N, em._p(u0_dev), em._p(p), int(ps is None)
    a.At, a.Qt, a.QLt = em._p(At), em._p(Qt), em._p(QLt)
    if adaptive is None:
        tg = np.ascontiguousarray(np.asarray(grid, float))
        hs = np.ascontiguousarray(np.diff(tg))
        nsteps = len(hs)
        n_save = nsteps + 1 if everystep else 1
        uniq, inv = np.unique(hs, return_inverse=True)
        ptab = np.zeros((len(uniq), lib().emul_tab_stride()))
        for k, h in enumerate(uniq):
            lib().emul_precond_fill(q, float(h), float(h) ** (-q - 1 / 2), em._p(ptab[k]))
        tab_idx = np.ascontiguousarray(inv.astype(np.int32))
        a.t0 = float(tg[0])
    else:
        tg = hs = ptab = np.zeros(1)
        tab_idx = np.zeros(1, np.int32)
        nsteps, n_save = 0, adaptive["max_save"]
        a.t0, a.t1, a.abstol, a.reltol, a.dt0 = (adaptive[k] for k in ("t0", "t1", "abstol", "reltol", "dt0"))
    a.hs, a.ptab, a.tab_idx, a.nsteps = em._p(hs), em._p(ptab), em._p(tab_idx, em.ip), nsteps
    a.ctrl, a.max_save = em._p(ctrl), n_save
    a.everystep, a.fixed_diffusion, a.want_loglik = int(everystep), MODELS[model], 1
    nd = d if mv else 1
    mean = np.zeros((n_save, D, N)); cov = np.zeros((n_save, TRI, N)); diff = np.zeros((n_save, nd, N))
    tsave = np.zeros((n_save, N)); loglik = np.zeros(N)
    ints = [np.zeros(N, np.int32) for _ in range(6)]
    a.mean, a.cov, a.diff, a.tsave, a.loglik = em._p(mean), em._p(cov), em._p(diff), em._p(tsave), em._p(loglik)
    a.naccept, a.nreject, a.nf, a.njac, a.nsaved, a.retcode = [em._p(x, em.ip) for x in ints]
    rc = lib().emul_filter_time(C.byref(a), em._p(tg), None if lin is None else em._p(np.ascontiguousarray(lin)), kernel)
    assert rc == 0, rc
    if model in ("fixed", "fixedMAP"):  # postamble! (src/integrator_utils.jl:4-18), the device's scale_cov_kernel
        cov *= diff[-1, 0][None, None, :]
        diff[1:] = diff[-1][None]
        loglik[:] = np.nan
    out = dict(mean=mean.transpose(2, 0, 1), cov=em.unpack_tril(cov.transpose(2, 0, 1), D), diff=diff.transpose(2, 0, 1),
               tsave=tsave.T, loglik=loglik, naccept=ints[0], nreject=ints[1], nsaved=ints[4], retcode=ints[5])
    if smooth and not mv:
        smean = np.zeros_like(mean); scov = np.zeros_like(cov)
        d1 = np.ascontiguousarray(diff[:, 0, :])
        a.diff = em._p(d1)
        a.smean, a.scov, a.n_save = em._p(smean), em._p(scov), n_save
        a.everystep = 3 if kernel == 2 else 1  # (the row-team smoother behind the row-team filter)
        assert lib().emul_smooth(C.byref(a), d) == 0
        out["smean"] = smean.transpose(2, 0, 1)
        out["scov"] = em.unpack_tril(scov.transpose(2, 0, 1), D)
        out["smean_dev"] = smean
    return out


def u0_pair():
    vf = tr.forced()
    return vf, np.stack([vf.u0, vf.u0 * 1.03 + 0.02])


@functools.lru_cache(maxsize=None)
def reference(kind, q, model, j, adaptive=False):
    vf, u0s = u0_pair()
    alg = orc.Alg(kind, q, model, True)
    if adaptive:
        return orc.solve(vf, alg, u0=u0s[j], tspan=(0.25, 1.25), adaptive=True, abstol=1e-6, reltol=1e-4, dt=1e-2)
    return orc.solve(vf, alg, u0=u0s[j], tspan=(GRID[0], GRID[-1]), tgrid=GRID)


@pytest.mark.parametrize("kernel", [0, 1, 2])
@pytest.mark.parametrize("model", ["dynamic", "fixed"])
@pytest.mark.parametrize("q", [1, 2, 3])
@pytest.mark.parametrize("kind", ["EK0", "EK1"])
def test_fixed_grid_kernels_match_reference(kind, q, model, kernel):
    vf, u0s = u0_pair()
    r = emul_time(q, kind == "EK1", u0s, vf.p, model, kernel, grid=GRID)
    for j in range(2):
        ref = reference(kind, q, model, j)
        assert r["retcode"][j] == 0
        np.testing.assert_allclose(r["mean"][j][0], ref.means(smoothed=False)[0], rtol=1e-13)  # the initialisation, f_t included
        np.testing.assert_allclose(r["mean"][j][:, :2], ref.means(smoothed=False)[:, :2], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(r["smean"][j][:, :2], ref.u, rtol=1e-10, atol=1e-12)
        assert P.cov_err(r["cov"][j], ref.covs(smoothed=False)) < 1e-6
        assert P.cov_err(r["scov"][j], ref.covs(smoothed=True)) < 1e-6
        np.testing.assert_allclose(r["diff"][j][1:, 0], ref.diffusions, rtol=1e-8)
        if model == "dynamic":
            np.testing.assert_allclose(r["loglik"][j], ref.log_likelihood, rtol=1e-9)


@pytest.mark.parametrize("kernel", [0, 2])
def test_final_state_mode_is_the_last_record(kernel):
    vf, u0s = u0_pair()
    every = emul_time(3, True, u0s, vf.p, "dynamic", kernel, grid=GRID, smooth=False)
    last = emul_time(3, True, u0s, vf.p, "dynamic", kernel, grid=GRID, everystep=False, smooth=False)
    np.testing.assert_array_equal(last["mean"][:, 0], every["mean"][:, -1])
    np.testing.assert_array_equal(last["cov"][:, 0], every["cov"][:, -1])


@pytest.mark.parametrize("kernel", [0, 2])
@pytest.mark.parametrize("q", [1, 2, 3])
@pytest.mark.parametrize("kind", ["EK0", "EK1"])
def test_adaptive_kernels_match_reference(kind, q, kernel):
    vf, u0s = u0_pair()
    r = emul_time(q, kind == "EK1", u0s, vf.p, "dynamic", kernel, smooth=False,
                  adaptive=dict(t0=0.25, t1=1.25, abstol=1e-6, reltol=1e-4, dt0=1e-2, max_save=4096))
    for j in range(2):
        ref = reference(kind, q, "dynamic", j, True)
        assert r["retcode"][j] == 0 and (r["naccept"][j], r["nreject"][j]) == (ref.naccept, ref.nreject)
        keep = np.arange(r["nsaved"][j])
        t = r["tsave"][j][keep]
        keep = keep[np.concatenate([[True], t[1:] != t[:-1]])]  # a rejected attempt repeats the record at the old time
        assert len(keep) == len(ref.t)
        np.testing.assert_allclose(r["tsave"][j][keep], ref.t, rtol=1e-8)
        np.testing.assert_allclose(r["mean"][j][keep][:, :2], ref.means(smoothed=False)[:, :2], rtol=1e-6, atol=1e-12)
        assert P.cov_err(r["cov"][j][keep], ref.covs(smoothed=False)) < 1e-4


@pytest.mark.parametrize("kernel", [0, 1, 2])
def test_ieks_two_iterations(kernel):
    """The IEKS step's Jacobian at (u_lin, tnew): iteration 1 is EK1, iteration 2 runs the IEKS kernels with the smoothed u of the
    first as linearisation points.  (The Jacobian of `forced`, diag(p0, p2 t), does not depend on u: both iterations give the same
    posterior, and what the second one checks is that the IEKS kernels evaluate it at the step's new time.)"""
    vf, u0s = u0_pair()
    q = 2
    first = emul_time(q, True, u0s, vf.p, "dynamic", kernel, grid=GRID)
    lin = np.ascontiguousarray(first["smean_dev"][:, :2, :])
    second = emul_time(q, True, u0s, vf.p, "dynamic", kernel, grid=GRID, lin=lin)
    for j in range(2):
        ref = ier.solve_ieks(vf, q, "dynamic", GRID, 2, u0=u0s[j], history=True)
        for got, want in ((first, ref[0]), (second, ref[1])):
            np.testing.assert_allclose(got["mean"][j][:, :2], want.means(smoothed=False)[:, :2], rtol=1e-10, atol=1e-12)
            np.testing.assert_allclose(got["smean"][j][:, :2], want.u, rtol=1e-10, atol=1e-12)
            np.testing.assert_allclose(got["loglik"][j], want.log_likelihood, rtol=1e-9)


@pytest.mark.parametrize("kernel", [0, 1])
def test_dynamic_mv_ek0(kernel):
    vf, u0s = u0_pair()
    q = 3
    r = emul_time(q, False, u0s, vf.p, "dynamicMV", kernel, grid=GRID)
    for j in range(2):
        ref = mvr.solve(vf, "dynamicMV", q, u0=u0s[j], tspan=(GRID[0], GRID[-1]), tgrid=GRID, smooth=False)
        np.testing.assert_allclose(r["mean"][j][:, :2], ref.means(smoothed=False)[:, :2], rtol=1e-10, atol=1e-12)
        assert P.cov_err(r["cov"][j], ref.covs(smoothed=False)) < 1e-6
        np.testing.assert_allclose(r["diff"][j][1:], np.array(ref.diffusions), rtol=1e-8)
        np.testing.assert_allclose(r["loglik"][j], ref.log_likelihood, rtol=1e-9)
