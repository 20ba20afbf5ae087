"""Per-trajectory parameters (`EnsembleProblem(..., ps=...)`, `params_shared = 0` in the C ABI) on every kernel family, each
checked trajectory against the oracle run on ITS row of `ps`.  Needs a real MI355X.

Every filter kernel family has its own loader `pl[k] = P.p_shared ? P.p[k] : P.p[k * N + i]`; the rest of the suite runs with
one shared parameter vector, which cannot see a wrong `i`, a transposed [n_params][N] layout or a wrong slice on the host: all
of those give finite, well-conditioned solutions of a neighbouring ODE.  No bar here is new: each test uses the ones the suite
already holds the same kernel to with shared parameters (named in its docstring), and first asserts from the oracle alone that
neighbouring rows of `ps` lie at least 1e-6 apart in the solution block (tests/_params.py), 10^4 times the bar of that block.
Every test asserts the name of the kernel it means to run.

With ODEF_PARAMS_RATIOS set to a file name, the error / tolerance ratios of the oracle-parity tests are appended there as
JSON lines (profiles/r05_params_ratios.jsonl is such a run)."""
import json
import os

import numpy as np
import pytest

import _errors_reference as er
import _ieks_reference as ier
import _mv_reference as mvr
import _params as PP
import _parity as P
import _time_reference as tr
import odefilter_oracle as orc

pytestmark = pytest.mark.gpu

N = 131  # 2 wavefronts + 3 lanes; 8 teams of 16 + 3
TRAJS = (0, 15, 16, 63, 64, 127, 128, 130)
FILTER_KERNELS = {"lane": "0", "rows": "1000000000"}  # ODEF_FILTER_ROWS_MAX_N, as tests/test_gpu_parity.py
FIXED_NAME = {"lane": "ek_filter_fixed_kernel", "rows": "ek_filter_rows_kernel"}
ADAPTIVE_NAME = {"lane": "ek_filter_adaptive_kernel", "rows": "ek_filter_rows_adaptive_kernel"}

_ENSEMBLES = {}
_RATIOS = []


def _ensemble(rhs, n):
    """(vf, u0s [n, d], ps [n, n_params]) of a compiled-in field, made once: p (1 + 0.05 x standard normal)."""
    if (rhs, n) not in _ENSEMBLES:
        vf = tr.forced() if rhs == "forced" else orc.vector_field(rhs)
        _ENSEMBLES[rhs, n] = (vf,) + PP.ensemble(vf, n, seed=11)
    return _ENSEMBLES[rhs, n]


def _problem(pkg, name, vf, tspan, u0s, ps):
    return pkg.EnsembleProblem(pkg.ODEProblem(name, vf.u0, tspan, vf.p), u0s=u0s, ps=ps)


@pytest.fixture(scope="module", autouse=True)
def _write_ratios():
    yield
    out = os.environ.get("ODEF_PARAMS_RATIOS")
    if out and _RATIOS:
        with open(out, "a") as f:
            for r in _RATIOS:
                f.write(json.dumps(r) + "\n")


def _oracle_parity(case, i, mean, cov, vf, alg_o, u0, kw, smoothed):
    """P.check_against_oracle of one trajectory's records against the oracle on `kw["p"]`; the ratios are kept for the record."""
    base, nm, nc = P.oracle_noise(vf, alg_o, u0, kw, smoothed)
    be, ce = P.check_against_oracle(mean, cov, base.means(smoothed=smoothed), base.covs(smoothed=smoothed), vf.d, nm, nc,
                                   f"{case} traj {i} smoothed={smoothed}")
    tol = np.maximum(P.FLOOR, P.NOISE_FACTOR * nm)
    tol[0] = P.U_RTOL
    _RATIOS.append({"case": case, "traj": int(i), "smoothed": bool(smoothed), "block_ratio": [float(f"{x:.3g}") for x in be / tol],
                    "cov_ratio": float(f"{ce / max(1e-9, P.NOISE_FACTOR * nc):.3g}")})
    return base


def _separated_fixed(vf, alg_o, u0s, ps, trajs, kw, what):
    """Section 3 of the module docstring for a fixed-grid case; the own-row solutions are the cached ones of P.oracle_noise."""
    filt = orc.Alg(alg_o.kind, alg_o.order, alg_o.diffusionmodel, False)
    PP.assert_separated(lambda u0, p: orc.solve(vf, filt, u0=u0, p=p, **kw).means(smoothed=False), u0s, ps, trajs, vf.d, what,
                        base=lambda i: P.oracle_noise(vf, alg_o, u0s[i], dict(kw, p=ps[i]), False)[0].means(smoothed=False))


# ---- lane and row-team filters, fixed grid ------------------------------------------------------------------------------------

FIXED = [
    # rhs, kind, order, dt (32 steps)
    ("lorenz63", "EK1", 3, 2.0**-8),
    ("lotka_volterra", "EK0", 2, 2.0**-7),  # d = 2, four parameters
    ("vanderpol", "EK1", 4, 2.0**-7),       # one parameter, mu = 1
]


@pytest.mark.parametrize("family", ["lane", "rows"])
@pytest.mark.parametrize("rhs,kind,q,dt", FIXED, ids=[f"{c[0]}-{c[1]}{c[2]}" for c in FIXED])
def test_fixed_grid_filters_against_oracle(pkg, monkeypatch, rhs, kind, q, dt, family):
    """ek_lane.h filter_fixed_lane and rows_filter.h rows_initial_state / rows_filter_fixed: filter and smoothed records at the
    bars of test_ensemble_parity_with_oracle, the log-likelihood at 1e-8 as test_config1_fhn_ek0_full."""
    monkeypatch.setenv("ODEF_FILTER_ROWS_MAX_N", FILTER_KERNELS[family])
    monkeypatch.setenv("ODEF_FILTER_LAG_MAX_N", "0")  # the lane filter as large ensembles run it: records stored within the step
    vf, u0s, ps = _ensemble(rhs, N)
    kw = dict(tspan=(0.0, 32 * dt), dt=dt)
    sol = pkg.solve(_problem(pkg, rhs, vf, kw["tspan"], u0s, ps), (pkg.EK1 if kind == "EK1" else pkg.EK0)(order=q), pkg.EnsembleHIP(),
                    dt=dt, adaptive=False)
    assert FIXED_NAME[family] in sol.ctx.kernel_name(0), sol.ctx.kernel_name(0)
    assert family == "rows" or sol.ctx.kernel_name(0).endswith("false>"), sol.ctx.kernel_name(0)
    assert sol.retcode == ["Success"] * N and len(sol.t) == 33
    alg_o = orc.Alg(kind, q, "dynamic", True)
    _separated_fixed(vf, alg_o, u0s, ps, TRAJS, kw, f"{rhs} {kind}({q})")
    mf, cf, ms, cs = sol.x_filt_mean(), sol.x_filt_cov(), sol.x_smooth_mean(), sol.x_smooth_cov()
    for i in TRAJS:
        for smoothed, (m, c) in ((False, (mf, cf)), (True, (ms, cs))):
            base = _oracle_parity(f"{rhs} {kind}({q}) {family}", i, m[i], c[i], vf, alg_o, u0s[i], dict(kw, p=ps[i]), smoothed)
        np.testing.assert_array_equal(sol.t, base.t)
        np.testing.assert_allclose(sol.log_likelihood[i], base.log_likelihood, rtol=1e-8)
    sol.ctx.close()


# ---- lane and row-team filters, adaptive ----------------------------------------------------------------------------------------


@pytest.mark.parametrize("family", ["lane", "rows"])
@pytest.mark.parametrize("rhs,q", [("lorenz63", 3), ("lotka_volterra", 2)])
def test_adaptive_filters_against_oracle(pkg, monkeypatch, rhs, q, family):
    """ek_lane.h filter_adaptive_lane and rows_filter.h rows_filter_adaptive at the bars of test_static_diffusion_models: the
    oracle's accepted and rejected steps, t and u at 1e-6."""
    monkeypatch.setenv("ODEF_FILTER_ROWS_MAX_N", FILTER_KERNELS[family])
    vf, u0s, ps = _ensemble(rhs, N)
    t1 = 0.5
    kw = dict(adaptive=True, dt=2.0**-8)
    sol = pkg.solve(_problem(pkg, rhs, vf, (0.0, t1), u0s, ps), pkg.EK1(order=q), pkg.EnsembleHIP(), max_steps=256, **kw)
    assert ADAPTIVE_NAME[family] in sol.ctx.kernel_name(0), sol.ctx.kernel_name(0)
    assert sol.retcode == ["Success"] * N
    alg_o = orc.EK1(order=q, smooth=True)
    for i in (0, 64, 130):
        ref = orc.solve(vf, alg_o, u0=u0s[i], p=ps[i], tspan=(0.0, t1), **kw)
        other = orc.solve(vf, alg_o, u0=u0s[i], p=ps[(i + 1) % N], tspan=(0.0, t1), **kw)
        assert PP.separation_adaptive(other, ref, vf.d) >= PP.MIN_SEPARATION, i
        n = len(ref.t)
        assert int(sol.nsaved[i]) == n and int(sol.destats.nreject[i]) == ref.nreject, i
        np.testing.assert_allclose(sol.t[i, :n], ref.t, rtol=1e-6)
        np.testing.assert_allclose(sol.x_filt_mean()[i, :n, : vf.d], ref.means(smoothed=False)[:, : vf.d], rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(sol.u[i, :n], ref.u, rtol=1e-6, atol=1e-12)
        assert sol.t[i, n - 1] == t1
    sol.ctx.close()


# ---- the wave -> trajectory map of the fixed-step lane filter ---------------------------------------------------------------------


def test_wave_map_with_per_trajectory_parameters(pkg, monkeypatch):
    """ek_lane.h takes its trajectory index from wave_first_trajectory: with 10 blocks map 1 is not the identity, so a loader
    that indexed `ps` with the unmapped block would pass every other test of this file.  Both maps give the same bits (the
    field list of tests/test_wave_map.py); under map 1 the first and last lanes of moved waves, and the lane of the partial
    one, agree with the oracle."""
    import test_wave_map as wm

    monkeypatch.setenv("ODEF_FILTER_ROWS_MAX_N", "0")
    n = 577
    vf, u0s, ps = _ensemble("lorenz63", n)
    out = {}
    for mode in (0, 1):
        monkeypatch.setenv("ODEF_WAVE_MAP", str(mode))
        with pkg.Context("lorenz63", 3, 1, n, smooth=True, save_everystep=True, want_loglik=True, params_shared=False) as ctx:
            ctx.set_problem(u0s, ps, 0.0)
            ctx.solve_fixed(wm.GRID)
            assert "ek_filter_fixed_kernel" in ctx.kernel_name(0), ctx.kernel_name(0)
            ctx.smooth()
            out[mode] = {name: ctx.get(f).copy() for name, f in {**wm.F_RECORDS, **wm.F_SMOOTHED}.items()}
    a, b = out[0], out[1]
    assert (a["RETCODE"] == 0).all() and (a["NSAVED"] == wm.NSTEPS + 1).all() and np.isfinite(a["MEAN"]).all()
    wm._assert_same_bits(a, b, "N = 577, per-trajectory parameters")
    alg_o = orc.Alg("EK1", 3, "dynamic", True)
    kw = dict(tspan=(0.0, wm.NSTEPS * wm.DT), dt=wm.DT)
    trajs = (0, 63, 64, 511, 512, 576)
    _separated_fixed(vf, alg_o, u0s, ps, trajs, kw, "lorenz63 EK1(3), 8 steps")
    for i in trajs:
        for smoothed, (m, c) in ((False, ("MEAN", "COV_TRIL")), (True, ("SMOOTH_MEAN", "SMOOTH_COV_TRIL"))):
            _oracle_parity("lorenz63 EK1(3) wave map 1", i, b[m][:, :, i], pkg.unpack_tril(b[c][:, :, i], 12), vf, alg_o, u0s[i],
                           dict(kw, p=ps[i]), smoothed)


# ---- the matrix-core filters ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("q", [2, 3])
def test_lorenz96_fixed_grid_on_the_matrix_cores(pkg, q):
    """filter_mfma.h, fixed grid (forcing 8 (1 +- 5 %) per trajectory): the assertions of
    test_lorenz96_on_the_matrix_core_kernels for trajectories 0 and 4."""
    n, ns, dt = 5, 12, 2.0**-7
    vf, u0s, ps = _ensemble("lorenz96", n)
    kw = dict(tspan=(0.0, ns * dt), dt=dt)
    sol = pkg.solve(_problem(pkg, "lorenz96", vf, kw["tspan"], u0s, ps), pkg.EK1(order=q), pkg.EnsembleHIP(), dt=dt, adaptive=False)
    assert sol.retcode == ["Success"] * n
    assert "ek_filter_mfma_kernel<odef::RhsLorenz96" in sol.ctx.kernel_name(0), sol.ctx.kernel_name(0)
    assert "rts_smooth_sweeps_kernel<16" in sol.ctx.kernel_name(1) or "rts_smooth_mfma_kernel<16" in sol.ctx.kernel_name(1)
    alg_o = orc.Alg("EK1", q, "dynamic", True)
    _separated_fixed(vf, alg_o, u0s, ps, (0, 4), kw, f"lorenz96 EK1({q})")
    mf, ms, cf, cs = sol.x_filt_mean(), sol.x_smooth_mean(), sol.x_filt_cov(), sol.x_smooth_cov()
    for i in (0, 4):
        for smoothed, m, c in ((False, mf, cf), (True, ms, cs)):
            base = _oracle_parity(f"lorenz96 EK1({q}) mfma", i, m[i], c[i], vf, alg_o, u0s[i], dict(kw, p=ps[i]), smoothed)
        for c in (cf[i][-1], cs[i][1]):
            w = np.linalg.eigvalsh(c)
            assert w.min() >= -1e-9 * np.abs(w).max()
        np.testing.assert_allclose(sol.log_likelihood[i], base.log_likelihood, rtol=1e-6)
    sol.ctx.close()


@pytest.mark.parametrize("q", [2, 3])
def test_lorenz96_adaptive_on_the_matrix_cores(pkg, q):
    """filter_mfma.h, adaptive: settings and bars of test_lorenz96_adaptive_dense_output_and_sampling, the filter part."""
    n, t1 = 5, 0.1
    vf, u0s, ps = _ensemble("lorenz96", n)
    kw = dict(dt=2.0**-8, adaptive=True, abstol=1e-8, reltol=1e-6)
    sol = pkg.solve(_problem(pkg, "lorenz96", vf, (0.0, t1), u0s, ps), pkg.EK1(order=q, smooth=False), pkg.EnsembleHIP(), max_steps=256, **kw)
    assert sol.retcode == ["Success"] * n
    assert "ek_filter_mfma_adaptive_kernel<odef::RhsLorenz96" in sol.ctx.kernel_name(0), sol.ctx.kernel_name(0)
    alg_o = orc.EK1(order=q, smooth=False)
    for i in (0, 4):
        ref = orc.solve(vf, alg_o, u0=u0s[i], p=ps[i], tspan=(0.0, t1), **kw)
        other = orc.solve(vf, alg_o, u0=u0s[i], p=ps[(i + 1) % n], tspan=(0.0, t1), **kw)
        assert PP.separation_adaptive(other, ref, 16) >= PP.MIN_SEPARATION, i
        k = len(ref.t)
        assert int(sol.nsaved[i]) == k and int(sol.destats.nreject[i]) == ref.nreject
        np.testing.assert_allclose(sol.t[i][:k], ref.t, rtol=1e-6)
        np.testing.assert_allclose(sol.u[i][:k], ref.u, rtol=1e-6, atol=1e-9)
    sol.ctx.close()


def test_run_time_field_on_the_matrix_cores(pkg):
    """The run-time compiled module of test_user_vector_field_on_the_matrix_core_kernels (Lorenz-96, d = 12, order 2, its one
    parameter the forcing) brings its own copy of the loader: fixed grid, filter and smoother, at that test's bars."""
    import test_gpu_parity as tgp

    d, q, name = 12, 2, "UserL96d12"
    pkg.compile_rhs(name, tgp._l96_source(name, d), d, 1)

    def f(u, p, t):
        return [(u[(i + 1) % d] - u[(i + d - 2) % d]) * u[(i + d - 1) % d] - u[i] + p[0] for i in range(d)]

    def jac(u, p, t):
        J = np.zeros((d, d))
        for i in range(d):
            ip, im2, im1 = (i + 1) % d, (i + d - 2) % d, (i + d - 1) % d
            J[i, ip] += u[im1]
            J[i, im2] -= u[im1]
            J[i, im1] += u[ip] - u[im2]
            J[i, i] -= 1.0
        return J

    u0 = np.array([1.0, 2.0, 0.5, -1.0, 0.3, 1.5, -0.7, 0.9, 1.2, -0.4, 0.8, 2.1])
    vf = orc.VectorField(name, 100, d, 1, f, jac, u0, np.array([8.0]), (0.0, 0.1))
    n, ns, dt = 3, 12, 2.0**-7
    u0s, ps = PP.ensemble(vf, n, seed=11)
    kw = dict(tspan=(0.0, ns * dt), dt=dt)
    sol = pkg.solve(_problem(pkg, name, vf, kw["tspan"], u0s, ps), pkg.EK1(order=q), pkg.EnsembleHIP(), dt=dt, adaptive=False)
    assert sol.retcode == ["Success"] * n
    assert f"ek_filter_mfma_kernel<odef::{name}" in sol.ctx.kernel_name(0), sol.ctx.kernel_name(0)
    alg_o = orc.Alg("EK1", q, "dynamic", True)
    _separated_fixed(vf, alg_o, u0s, ps, (0, 2), kw, "user L96 d=12")
    mf, ms, cf, cs = sol.x_filt_mean(), sol.x_smooth_mean(), sol.x_filt_cov(), sol.x_smooth_cov()
    for i in (0, 2):
        for smoothed, m, c in ((False, mf, cf), (True, ms, cs)):
            _oracle_parity("user L96 d=12 EK1(2) mfma", i, m[i], c[i], vf, alg_o, u0s[i], dict(kw, p=ps[i]), smoothed)
    sol.ctx.close()


# ---- kernels that share the loader but are their own instantiations ------------------------------------------------------------

N_SMALL = 70


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.nanmax(np.abs(a - b)) / (np.nanmax(np.abs(b)) + 1e-300))


@pytest.mark.parametrize("family", ["lane", "rows"])
def test_ieks_two_iterations(pkg, monkeypatch, family):
    """ek_filter_fixed_ieks_kernel / ek_filter_rows_ieks_kernel at the bars of test_ieks_parity (tests/test_gpu_ieks.py)."""
    monkeypatch.setenv("ODEF_FILTER_ROWS_MAX_N", FILTER_KERNELS[family])
    vf, u0s, ps = _ensemble("lorenz63", N_SMALL)
    q, dt, t1 = 3, 2.0**-7, 0.25
    grid = pkg.fixed_time_grid(0.0, t1, dt)
    sol = pkg.solve_ieks(_problem(pkg, "lorenz63", vf, (0.0, t1), u0s, ps), pkg.IEKS(order=q), pkg.EnsembleHIP(), dt=dt, adaptive=False,
                         iterations=2)
    assert {"lane": "ek_filter_fixed_ieks_kernel", "rows": "ek_filter_rows_ieks_kernel"}[family] in sol.ctx.kernel_name(0)
    assert sol.retcode == ["Success"] * N_SMALL

    def ref(u0, p):
        return ier.solve_ieks(vf, q, "dynamic", grid, 2, u0=u0, p=p)

    refs = {i: ref(u0s[i], ps[i]) for i in (0, N_SMALL - 1)}
    PP.assert_separated(lambda u0, p: ref(u0, p).means(smoothed=True), u0s, ps, refs, vf.d, "IEKS lorenz63",
                        base=lambda i: refs[i].means(smoothed=True))
    for i, r in refs.items():
        assert _rel(sol.x_smooth_mean()[i], r.means(smoothed=True)) < 1e-9, i
        assert _rel(sol.x_filt_mean()[i], r.means(smoothed=False)) < 1e-9, i
        assert _rel(sol.x_smooth_cov()[i], r.covs(smoothed=True)) < 1e-6, i
        assert abs(sol.log_likelihood[i] - r.log_likelihood) <= 1e-7 * abs(r.log_likelihood)
    sol.ctx.close()


@pytest.mark.parametrize("adaptive", [False, True], ids=["fixed", "adaptive"])
def test_dynamic_mv_ek0(pkg, adaptive):
    """ek_filter_fixed_mv_kernel / ek_filter_adaptive_mv_kernel at the bars of test_mv_parity (q <= 3)."""
    vf, u0s, ps = _ensemble("lorenz63", N_SMALL)
    q, t1, d = 3, 0.25, 3
    kw = dict(adaptive=True, dt=2.0**-8) if adaptive else dict(adaptive=False, dt=2.0**-6)
    sol = pkg.solve(_problem(pkg, "lorenz63", vf, (0.0, t1), u0s, ps), pkg.EK0(order=q, diffusionmodel="dynamicMV"), pkg.EnsembleHIP(),
                    **kw, **({"max_steps": 256} if adaptive else {}))
    assert ("ek_filter_adaptive_mv_kernel" if adaptive else "ek_filter_fixed_mv_kernel") in sol.ctx.kernel_name(0)
    assert sol.retcode == ["Success"] * N_SMALL
    for i in (0, N_SMALL - 1):
        ref = mvr.solve(vf, "dynamicMV", q, u0=u0s[i], p=ps[i], tspan=(0.0, t1), **kw)
        other = mvr.solve(vf, "dynamicMV", q, u0=u0s[i], p=ps[(i + 1) % N_SMALL], tspan=(0.0, t1), **kw)
        assert PP.separation_adaptive(other, ref, d) >= PP.MIN_SEPARATION, i
        n = len(ref.t)
        assert int(sol.nsaved[i]) == n
        if adaptive:
            assert (int(sol.destats.naccept[i]), int(sol.destats.nreject[i])) == (ref.naccept, ref.nreject)
            np.testing.assert_allclose(sol.t[i, :n], ref.t, rtol=1e-8)
        rt = 1e-6 if adaptive else 1e-10
        np.testing.assert_allclose(sol.x_filt_mean()[i, :n, :d], ref.means(smoothed=False)[:, :d], rtol=rt, atol=1e-12)
        np.testing.assert_allclose(sol.u[i, :n], ref.u, rtol=rt, atol=1e-12)
        assert _rel(sol.diffusions[i, : n - 1], np.array(ref.diffusions)) < (1e-5 if adaptive else 1e-8)
        assert P.cov_err(sol.x_filt_cov()[i, :n], ref.covs(smoothed=False)) < (1e-4 if adaptive else 1e-6)
        assert P.cov_err(sol.x_smooth_cov()[i, :n], ref.covs(smoothed=True)) < (1e-4 if adaptive else 1e-6)
        np.testing.assert_allclose(sol.log_likelihood[i], ref.log_likelihood, rtol=1e-5 if adaptive else 1e-9)
    sol.ctx.close()


FORCED_TSPAN, FORCED_DT = (0.25, 0.75), 2.0**-6  # 32 steps, from the non-zero t0 of the field


@pytest.mark.parametrize("family", ["lane", "rows"])
def test_time_dependent_field(pkg, monkeypatch, family):
    """The instantiations around f(u, p, t) (the compiled-in `forced`) at the fixed-grid bars of tests/test_gpu_time.py."""
    monkeypatch.setenv("ODEF_FILTER_ROWS_MAX_N", FILTER_KERNELS[family])
    vf, u0s, ps = _ensemble("forced", N_SMALL)
    sol = pkg.solve(_problem(pkg, "forced", vf, FORCED_TSPAN, u0s, ps), pkg.EK1(order=3), pkg.EnsembleHIP(), dt=FORCED_DT, adaptive=False)
    name = sol.ctx.kernel_name(0)
    assert FIXED_NAME[family] in name and "RhsForced" in name, name
    assert sol.retcode == ["Success"] * N_SMALL
    alg_o = orc.Alg("EK1", 3, "dynamic", True)

    def ref(u0, p):
        return orc.solve(vf, alg_o, u0=u0, p=p, tspan=FORCED_TSPAN, dt=FORCED_DT)

    refs = {i: ref(u0s[i], ps[i]) for i in (0, N_SMALL - 1)}
    PP.assert_separated(lambda u0, p: ref(u0, p).means(smoothed=False), u0s, ps, refs, 2, "forced", base=lambda i: refs[i].means(smoothed=False))
    for i, r in refs.items():
        n = len(r.t)
        assert n == 33 and int(sol.nsaved[i]) == n
        np.testing.assert_allclose(sol.x_filt_mean()[i, :n, :2], r.means(smoothed=False)[:, :2], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(sol.u[i, :n], r.u, rtol=1e-10, atol=1e-12)
        assert P.cov_err(sol.x_filt_cov()[i, :n], r.covs(smoothed=False)) < 1e-6
        assert P.cov_err(sol.x_smooth_cov()[i, :n], r.covs(smoothed=True)) < 1e-6
        assert abs(sol.log_likelihood[i] - r.log_likelihood) <= 1e-9 * abs(r.log_likelihood)
    sol.ctx.close()


def test_run_time_field_equals_the_compiled_in_one(pkg):
    """A compile_rhs copy of `forced` solved with `ps`: what test_run_time_field_equals_the_compiled_in_one (tests/test_gpu_time.py)
    asserts, fixed grid and adaptive."""
    import test_gpu_time as tgt

    pkg.compile_rhs("TimeForced", tgt.FORCED_SRC.replace("NAME", "TimeForced").replace("JAC", tgt.FORCED_JAC), 2, 3)
    vf, u0s, ps = _ensemble("forced", N_SMALL)
    for kw in (dict(dt=FORCED_DT, adaptive=False), dict(tgt.ADAPT, max_steps=256)):
        a = pkg.solve(_problem(pkg, "forced", vf, FORCED_TSPAN, u0s, ps), pkg.EK1(order=3), pkg.EnsembleHIP(), **kw)
        b = pkg.solve(_problem(pkg, "TimeForced", vf, FORCED_TSPAN, u0s, ps), pkg.EK1(order=3), pkg.EnsembleHIP(), **kw)
        assert "RhsForced" in a.ctx.kernel_name(0) and "TimeForced" in b.ctx.kernel_name(0)
        assert b.ctx.kernel_name(0) == a.ctx.kernel_name(0).replace("RhsForced", "TimeForced")
        np.testing.assert_array_equal(a.nsaved, b.nsaved)
        np.testing.assert_allclose(b.x_filt_mean(), a.x_filt_mean(), rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(b.x_smooth_mean(), a.x_smooth_mean(), rtol=1e-13, atol=1e-300)
        if not kw["adaptive"]:  # ... and neither is the run with every row's p = vf.p
            c = pkg.solve(_problem(pkg, "TimeForced", vf, FORCED_TSPAN, u0s, np.tile(vf.p, (N_SMALL, 1))), pkg.EK1(order=3), pkg.EnsembleHIP(), **kw)
            assert _rel(c.x_filt_mean()[..., :2], b.x_filt_mean()[..., :2]) > PP.MIN_SEPARATION
            c.ctx.close()
        a.ctx.close()
        b.ctx.close()


# ---- the `analytic` evaluation of the errors kernels ---------------------------------------------------------------------------


@pytest.mark.parametrize("adaptive", [False, True], ids=["fixed", "adaptive"])
def test_errors_against_the_analytic_solution_of_each_row(pkg, adaptive):
    """errors_kernels.h evaluates RhsLinear::analytic with its own copy of the loader: u* = u0_i exp(p_i t).  sol.u_analytic
    against the extended-precision truth of (u0s[i], ps[i]) at 4 ulp, sol.errors of the filter and the smoothed records through
    _errors_reference.check (DEVICE_FACTOR), as test_linear_against_its_analytic_solution."""
    from odefilters_jl_amd import host as h

    vf, u0s, ps = _ensemble("linear", N)
    nxt = np.roll(ps, -1, axis=0)
    t_end = np.array([1.0])
    apart = np.abs(er.linear_truth(u0s, nxt, t_end) - er.linear_truth(u0s, ps, t_end)).astype(float)[0]
    assert (apart.max(axis=0) / np.abs(u0s).max() >= PP.MIN_SEPARATION).all()
    kw = dict(adaptive=True, dt=1.0, abstol=1e-7, reltol=1e-5, max_steps=2048) if adaptive else dict(adaptive=False, dt=2.0**-5)
    sol = pkg.solve(_problem(pkg, "linear", vf, (0.0, 1.0), u0s, ps), pkg.EK1(order=2), pkg.EnsembleHIP(), **kw)
    ctx = sol.ctx
    assert sol.retcode == ["Success"] * N
    assert "ek_filter_rows" in ctx.kernel_name(0) and "RhsLinear" in ctx.kernel_name(0), ctx.kernel_name(0)
    t = ctx.get(h.F_T).reshape(ctx.n_save, N) if adaptive else ctx.get(h.F_T)
    truth = er.linear_truth(u0s, ps, t)
    got = {}
    for source in (0, 1):
        mean, cov = ctx.get((h.F_MEAN, h.F_SMOOTH_MEAN)[source]), ctx.get((h.F_COV_TRIL, h.F_SMOOTH_COV_TRIL)[source])
        ts, ns = (t, ctx.get(h.F_NSAVED)) if adaptive else (None, None)
        ref = er.evaluate(mean, cov, 2, truth, ts, ns)
        e = ctx.solution_errors(source)
        got[source] = {"final": e["final"], "l2": e["l2"], "linf": e["l∞"], "chi2": e["chi2"], "nused": e["nused"]}
        r = er.check(got[source], ref, er.unit_bounds(mean, cov, 2, truth, ref, ts, ns), label=f"linear, ps, source {source}")
        print(f"linear EK1(2) ps {'adaptive' if adaptive else 'fixed'} source {source}: error / unit bound", {k: f"{v:.3g}" for k, v in r.items()})
    assert ctx.kernel_name(3) == "odef::errors_partial_kernel<2, odef::TruthAnalytic<odef::RhsLinear>>"
    for key, mine in (("final", "final"), ("l2", "l2"), ("l∞", "linf")):  # sol.errors: those of sol.u, the smoothed records
        np.testing.assert_array_equal(sol.errors[key], got[1][mine])
    ua = sol.u_analytic  # [N, n_save, 2], every trajectory's kept records first
    for i in range(N):
        n = int(sol.nsaved[i])
        ti = sol.t[i, :n] if adaptive else sol.t
        want = er.linear_truth(u0s[i : i + 1], ps[i : i + 1], ti).astype(float)[:, :, 0]
        assert np.all(np.abs(ua[i, :n] - want) <= 4 * er.U * np.abs(want)), i
    if adaptive:
        assert int(sol.destats.nreject.sum()) > 0
    ctx.close()


# ---- entry points ---------------------------------------------------------------------------------------------------------------

RECORDS = (0, 1, 2, 4, 9, 10)  # MEAN, COV_TRIL, DIFFUSION, LOGLIK, NSAVED, RETCODE


def test_set_problem_device_takes_the_device_layout(pkg):
    """odef_set_problem_device with u0 [d][N] and p [n_params][N] in device memory: the bits of odef_set_problem with the host
    arrays [N][d], [N][n_params] (whose transposition is the other way into the same layout)."""
    import torch

    vf, u0s, ps = _ensemble("lorenz63", N)
    grid = np.arange(17) * 2.0**-8
    out = []
    for on_device in (False, True):
        with pkg.Context("lorenz63", 3, 1, N, params_shared=False) as ctx:
            if on_device:
                du0 = torch.from_numpy(np.ascontiguousarray(u0s.T)).to("cuda")
                dp = torch.from_numpy(np.ascontiguousarray(ps.T)).to("cuda")
                torch.cuda.synchronize()
                ctx.set_problem_device(du0.data_ptr(), dp.data_ptr(), 0.0)
            else:
                ctx.set_problem(u0s, ps, 0.0)
            ctx.solve_fixed(grid)
            assert "ek_filter_rows_kernel<odef::RhsLorenz63" in ctx.kernel_name(0), ctx.kernel_name(0)
            assert (ctx.get(10) == 0).all()
            out.append({f: ctx.get(f).copy() for f in RECORDS + (13,)})
    np.testing.assert_array_equal(out[0][13], u0s.T)
    for f in RECORDS + (13,):
        np.testing.assert_array_equal(out[1][f], out[0][f], err_msg=f"field {f}")
    # ... and those are the solutions of the rows of ps
    for i in (0, 64, 130):
        ref = orc.solve(vf, orc.EK1(order=3, smooth=False), u0=u0s[i], p=ps[i], tgrid=grid, tspan=(0.0, grid[-1]))
        other = orc.solve(vf, orc.EK1(order=3, smooth=False), u0=u0s[i], p=ps[(i + 1) % N], tgrid=grid, tspan=(0.0, grid[-1]))
        assert PP.separation(other.u, ref.u, 3) >= PP.MIN_SEPARATION
        np.testing.assert_allclose(out[1][0][:, :3, i], ref.u, rtol=1e-10)


@pytest.mark.parametrize("adaptive", [False, True], ids=["fixed", "adaptive"])
def test_group_shards_take_their_rows_of_the_parameters(pkg, adaptive):
    """DeviceGroup(params_shared=False): odef_group_set_problem hands every shard its rows of p [N][n_params].  Two shards on one
    device, 131 = 66 + 65, against ONE context of all 131, exactly as test_group_two_shards_equal_one_solve asserts."""
    from odefilters_jl_amd import host

    vf, u0s, ps = _ensemble("lorenz63", N)
    grid = np.arange(33) * 2.0**-9
    with host.DeviceGroup("lorenz63", 3, 1, N, 2, device_ids=[0, 0], params_shared=False) as grp:
        assert grp.shard(0) == (0, 66) and grp.shard(1) == (66, 65)
        grp.set_problem(u0s, ps, 0.0)
        if adaptive:
            grp.solve_adaptive(0.25, dt0=2.0**-9, max_steps=256)
        else:
            grp.solve_fixed(grid)
        fin0 = grp.allgather(from_device=0)
        fin1 = grp.allgather(from_device=1)
        names = [pkg.Context.kernel_name(_Shard(grp, g), 0) for g in range(2)]
    assert all("ek_filter" in nm and ("adaptive" in nm) == adaptive for nm in names), names
    np.testing.assert_array_equal(fin0, fin1)
    with pkg.Context("lorenz63", 3, 1, N, params_shared=False) as ctx:
        ctx.set_problem(u0s, ps, 0.0)
        if adaptive:
            ctx.solve_adaptive(0.25, dt0=2.0**-9, max_steps=256)
            mean, ns = ctx.get(0), ctx.get(9)
            ref = np.stack([mean[ns[i] - 1, :, i] for i in range(N)], axis=1)
        else:
            ctx.solve_fixed(grid)
            ref = ctx.get(0)[-1]
    np.testing.assert_array_equal(fin0, ref)
    if not adaptive:  # the last row of the first shard, the first of the second: each the oracle's answer for its own p
        for i in (0, 65, 66, 130):
            r = orc.solve(vf, orc.EK1(order=3, smooth=False), u0=u0s[i], p=ps[i], tspan=(0.0, grid[-1]), dt=2.0**-9)
            np.testing.assert_allclose(fin0[:3, i], r.u[-1], rtol=1e-11)
            assert _rel(orc.solve(vf, orc.EK1(order=3, smooth=False), u0=u0s[i], p=ps[(i + 1) % N], tspan=(0.0, grid[-1]), dt=2.0**-9).u[-1],
                        r.u[-1]) >= PP.MIN_SEPARATION


class _Shard:
    """The context of shard g of a DeviceGroup, with what Context.kernel_name needs."""

    def __init__(self, grp, g):
        self.lib, self._h = grp.lib, grp.lib.odef_group_ctx(grp._h, g)

    def _chk(self, rc):
        assert rc == 0, self.lib.odef_last_error(self._h).decode()


def test_refusals(pkg):
    vf, u0s, ps = _ensemble("lotka_volterra", 7)
    with pkg.Context("lotka_volterra", 2, 1, 7, params_shared=False) as ctx:
        for bad in (ps.T, ps[:6], ps[:, :3], vf.p):
            with pytest.raises(pkg.OdefError, match="p must have shape"):
                ctx.set_problem(u0s, bad, 0.0)
        with pytest.raises(pkg.OdefError, match="needs params_shared = 1"):
            ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-2)
    with pkg.Context("lotka_volterra", 2, 1, 7) as ctx:
        with pytest.raises(pkg.OdefError, match="p must have shape"):
            ctx.set_problem(u0s, ps, 0.0)


# ---- row i is its own problem ---------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("family", ["lane", "rows"])
def test_row_i_is_its_own_problem(pkg, monkeypatch, family):
    """Row i of the ensemble solve against the one-trajectory solve of (u0s[i], shared p = ps[i]) on the same kernel: the lane
    kernel bit for bit (its arithmetic does not depend on the position, test_full_size_properties), the row-team kernel at
    1e-11 on the solution block, the bar that test uses across kernels."""
    monkeypatch.setenv("ODEF_FILTER_ROWS_MAX_N", FILTER_KERNELS[family])
    vf, u0s, ps = _ensemble("lorenz63", N)
    grid = np.arange(33) * 2.0**-8
    with pkg.Context("lorenz63", 3, 1, N, params_shared=False) as ctx:
        ctx.set_problem(u0s, ps, 0.0)
        ctx.solve_fixed(grid)
        assert FIXED_NAME[family] in ctx.kernel_name(0), ctx.kernel_name(0)
        ens = {f: ctx.get(f).copy() for f in RECORDS}
    assert (ens[10] == 0).all()
    for i in (0, 64, 130):
        with pkg.Context("lorenz63", 3, 1, 1) as ctx:
            ctx.set_problem(u0s[i : i + 1], ps[i], 0.0)
            ctx.solve_fixed(grid)
            assert FIXED_NAME[family] in ctx.kernel_name(0), ctx.kernel_name(0)
            one = {f: ctx.get(f).copy() for f in RECORDS}
        if family == "lane":
            for f in (0, 1, 2):
                np.testing.assert_array_equal(ens[f][..., i], one[f][..., 0], err_msg=f"field {f}, trajectory {i}")
            assert ens[4][i] == one[4][0]
        else:
            np.testing.assert_allclose(ens[0][:, :3, i], one[0][:, :3, 0], rtol=1e-11)
        j = (i + 1) % N  # ... and not its neighbour's
        assert _rel(ens[0][:, :3, j], one[0][:, :3, 0]) > PP.MIN_SEPARATION


def test_row_i_is_its_own_problem_on_the_matrix_cores(pkg):
    n, grid = 5, np.arange(13) * 2.0**-7
    vf, u0s, ps = _ensemble("lorenz96", n)
    with pkg.Context("lorenz96", 2, 1, n, params_shared=False) as ctx:
        ctx.set_problem(u0s, ps, 0.0)
        ctx.solve_fixed(grid)
        assert "ek_filter_mfma_kernel<odef::RhsLorenz96" in ctx.kernel_name(0), ctx.kernel_name(0)
        assert (ctx.get(10) == 0).all()
        ens = ctx.get(0).copy()
    for i in (0, 4):
        with pkg.Context("lorenz96", 2, 1, 1) as ctx:
            ctx.set_problem(u0s[i : i + 1], ps[i], 0.0)
            ctx.solve_fixed(grid)
            assert "ek_filter_mfma_kernel<odef::RhsLorenz96" in ctx.kernel_name(0), ctx.kernel_name(0)
            one = ctx.get(0).copy()
        np.testing.assert_allclose(ens[:, :16, i], one[:, :16, 0], rtol=1e-11)
