"""Per-trajectory parameters (p_shared = 0, P.p laid out [n_params][N]) through the host build of the device source: the
fixed-step lane filter, the row-team filter, the adaptive lane filter, and the time-dependent and IEKS instantiations, each
trajectory against the oracle run on ITS parameter row.  Every other emulation test hands the kernels one shared vector.
The GPU tests (test_gpu_params.py) repeat these on the real kernels (CPU only here)."""
import functools

import numpy as np
import pytest

import _emul as E
import _ieks_reference as ier
import _params as PP
import _parity as P
import _time_reference as tr
import test_ieks_emul as ieks_emul
import test_time_emul as time_emul

orc = E.orc

N = 67  # one full wavefront of lanes and three more
TRAJS = (0, 1, 63, 64, 66)
NSTEPS = 32

FIXED = [
    # rhs, alg, dt
    ("lorenz63", orc.EK1(order=3), 2.0**-8),
    ("lotka_volterra", orc.EK0(order=2), 2.0**-7),
]


@functools.lru_cache(maxsize=None)
def _ensemble(rhs):
    vf = tr.forced() if rhs == "forced" else orc.vector_field(rhs)
    u0s, ps = PP.ensemble(vf, N, seed=11)
    return vf, u0s, ps


@pytest.mark.parametrize("everystep", [1, 3], ids=["lane", "rows"])
@pytest.mark.parametrize("rhs,alg,dt", FIXED, ids=[f"{c[0]}-{c[1].kind}{c[1].order}" for c in FIXED])
def test_fixed_grid_filter_and_smoother(rhs, alg, dt, everystep):
    """filter_fixed_lane (everystep = 1) and rows_filter_fixed (everystep = 3), filter and smoothed records."""
    vf, u0s, ps = _ensemble(rhs)
    tg = np.arange(NSTEPS + 1) * dt
    r = E.emul_solve(vf.rhs_id, vf.d, alg.order, alg.kind == "EK1", u0s, vf.p, ps=ps, tgrid=tg, smooth=True, everystep=everystep)
    assert (r["retcode"] == 0).all()

    def kw(p):
        return dict(tspan=(0.0, float(tg[-1])), dt=dt, p=p)

    filt = orc.Alg(alg.kind, alg.order, "dynamic", False)
    PP.assert_separated(lambda u0, p: orc.solve(vf, filt, u0=u0, **kw(p)).means(smoothed=False), u0s, ps, TRAJS, vf.d,
                        f"{rhs} {alg.kind}({alg.order})")
    for i in TRAJS:
        for smoothed in (False, True):
            base, nm, nc = P.oracle_noise(vf, alg, u0s[i], kw(ps[i]), smoothed)
            np.testing.assert_array_equal(base.t, tg)
            mean, cov = (r["smean"][i], r["scov"][i]) if smoothed else (r["mean"][i], r["cov"][i])
            P.check_against_oracle(mean, cov, base.means(smoothed=smoothed), base.covs(smoothed=smoothed), vf.d, nm, nc,
                                   f"{rhs} {alg.kind}({alg.order}) everystep={everystep} traj {i} smoothed={smoothed}")
        np.testing.assert_allclose(r["loglik"][i], base.log_likelihood, rtol=1e-6)


@pytest.mark.parametrize("rhs,q", [("lorenz63", 3), ("lotka_volterra", 2)])
def test_adaptive_lane_filter(rhs, q):
    """filter_adaptive_lane at the bars of test_adaptive_matches_oracle_step_sequence (tests/test_emul_parity.py): the same
    accepted and rejected steps as the oracle's controller loop on ps[i], t at 1e-9 and the solution block at 1e-7."""
    vf, u0s, ps = _ensemble(rhs)
    alg = orc.EK1(order=q, smooth=True)
    kw = dict(adaptive=True, dt=2.0**-9, tspan=(0.0, 0.5))
    r = E.emul_solve(vf.rhs_id, vf.d, q, True, u0s, vf.p, ps=ps, adaptive=True, t0=0.0, t1=0.5, dt0=2.0**-9, max_save=512, smooth=True)
    refs = {i: orc.solve(vf, alg, u0=u0s[i], p=ps[i], **kw) for i in TRAJS}
    for i in TRAJS:
        other = orc.solve(vf, alg, u0=u0s[i], p=ps[(i + 1) % N], **kw)
        assert PP.separation_adaptive(other, refs[i], vf.d) >= PP.MIN_SEPARATION, i
    for i, sol in refs.items():
        n = r["nsaved"][i]
        assert n == len(sol.t) and r["nreject"][i] == sol.nreject and r["retcode"][i] == 0, i
        np.testing.assert_allclose(r["tsave"][i][:n], sol.t, rtol=1e-9)
        np.testing.assert_allclose(r["mean"][i][:n, : vf.d], sol.means(smoothed=False)[:, : vf.d], rtol=1e-7)
        np.testing.assert_allclose(r["smean"][i][:n, : vf.d], sol.means(smoothed=True)[:, : vf.d], rtol=1e-7)


@pytest.mark.parametrize("kernel", [0, 2], ids=["lane", "rows"])
def test_time_dependent_field(kernel):
    """The instantiations around f(u, p, t) (tests/emul/emul_time.cpp) at the bars of tests/test_time_emul.py."""
    vf, u0s, ps = _ensemble("forced")
    q, grid = 2, time_emul.GRID
    alg = orc.Alg("EK1", q, "dynamic", True)
    r = time_emul.emul_time(q, True, u0s, vf.p, "dynamic", kernel, grid=grid, ps=ps)

    def ref(u0, p):
        return orc.solve(vf, alg, u0=u0, p=p, tspan=(grid[0], grid[-1]), tgrid=grid)

    PP.assert_separated(lambda u0, p: ref(u0, p).means(smoothed=False), u0s, ps, TRAJS, 2, "forced")
    for i in TRAJS:
        want = ref(u0s[i], ps[i])
        assert r["retcode"][i] == 0
        np.testing.assert_allclose(r["mean"][i][0], want.means(smoothed=False)[0], rtol=1e-13)  # the initialisation, f_t included
        np.testing.assert_allclose(r["mean"][i][:, :2], want.means(smoothed=False)[:, :2], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(r["smean"][i][:, :2], want.u, rtol=1e-10, atol=1e-12)
        assert P.cov_err(r["cov"][i], want.covs(smoothed=False)) < 1e-6
        np.testing.assert_allclose(r["loglik"][i], want.log_likelihood, rtol=1e-9)


@pytest.mark.parametrize("kernel", [0, 2], ids=["lane", "rows"])
def test_ieks_two_iterations(kernel):
    """The IEKS instantiations (tests/emul/emul_ieks.cpp) at the bars of tests/test_ieks_emul.py, Lorenz-63 order 3."""
    vf, u0s, ps = _ensemble("lorenz63")
    q, iters = 3, 2
    grid = np.arange(NSTEPS + 1) * 2.0**-8
    got = ieks_emul.emul_ieks(vf.rhs_id, vf.d, q, u0s, vf.p, grid, "dynamic", iters, kernel, ps=ps)
    PP.assert_separated(lambda u0, p: ier.solve_ieks(vf, q, "dynamic", grid, iters, u0=u0, p=p).means(smoothed=True), u0s, ps, TRAJS,
                        vf.d, "IEKS lorenz63")
    for i in TRAJS:
        ref = ier.solve_ieks(vf, q, "dynamic", grid, iters, u0=u0s[i], p=ps[i], history=True)
        for k in range(iters):
            smean, mean, ll, njac = got[k]
            assert ieks_emul._rel(smean[i], ref[k].means(smoothed=True)) < 1e-9, (k, i)
            assert ieks_emul._rel(mean[i], ref[k].means(smoothed=False)) < 1e-9, (k, i)
            assert njac[i] == len(grid) - 1
            assert abs(ll[i] - ref[k].log_likelihood) <= 1e-8 * abs(ref[k].log_likelihood)
