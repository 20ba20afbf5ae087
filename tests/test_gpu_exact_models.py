"""The HIP kernels of fixedMAP, the MV diffusion models, IEKS and the time-dependent field `forced` (through the C ABI) against
EXTENDED-PRECISION evaluations of the reference algorithm (tests/golden/exact_model_*_ld.npz; generator `make_exact.py --models`,
cases `_exact_cases.MODEL_CASES`).  The question of tests/test_gpu_exact.py: is the device as close to the exact result of the
reference algorithm as the float64 reference is (factor 16, `_parity.check_against_exact_floored`) -- per derivative block, for
the covariances of every record, the diffusions (MV: every component) and the log-likelihood -- with every kernel family forced
by the launch-time overrides and asserted through odef_kernel_name.  The same cases pass in emulation first
(tests/test_exact_models_emul.py).  Needs a real MI355X: run with `-m gpu`."""
import numpy as np
import pytest

import _exact_cases as X
import _parity as P
import test_gpu_ieks as TI
import test_gpu_time as TT

pytestmark = pytest.mark.gpu

N = 70  # ragged for 64-lane wavefronts (lane kernels) and for the four-trajectory waves of the row-team kernels
CHECKED = (0, 1, 2, 3, 66, 67, 68, 69)  # the first wavefront / team wave and the ragged last ones
NT = X.SMALL_NTRAJ
LAG_ENV = {"lane_lag": "1000000000", "lane": "0"}  # ODEF_FILTER_LAG_MAX_N


def _dim(case):
    return X.MODEL_DIM[case[1]] * (case[3] + 1)


def _problem(pkg, case, fx):
    """The fixture's four trajectories, k at every index i with i % 4 == k, on the fixture's time span."""
    u0s = fx["u0s"][np.arange(N) % NT]
    vf = X.model_field(case)
    return pkg.EnsembleProblem(pkg.ODEProblem(case[1], u0s[0], (float(fx["t"][0]), float(fx["t"][-1])), vf.p), u0s=u0s)


def check_model(fx, sol, case, what):
    family, rhs, kind, q, diffusion, dt = case
    d = X.MODEL_DIM[rhs]
    with_loglik = diffusion in ("dynamic", "dynamicMV")
    assert sol.retcode == ["Success"] * N
    np.testing.assert_array_equal(sol.t, fx["t"])
    mf, cf, ms, cs = sol.x_filt_mean(), sol.x_filt_cov(), sol.x_smooth_mean(), sol.x_smooth_cov()
    diff, ll = sol.diffusions, sol.log_likelihood
    assert diff.shape == ((N, X.SMALL_NSTEPS, d) if family == "mv" else (N, X.SMALL_NSTEPS))
    ratios = []
    for i in CHECKED:
        k = i % NT
        ratios.append(P.check_against_exact_floored(fx, k, mf[i], cf[i], ms[i], cs[i], d, diffusions=diff[i],
                                                    loglik=ll[i] if with_loglik else None, what=f"{X.model_id(case)} {what} traj {i}"))
        if family == "forced":
            P.check_initial_record_floored(fx, k, mf[i], d, f"{X.model_id(case)} {what} traj {i}")
    if not with_loglik:
        assert np.isnan(ll).all()  # src/integrator_utils.jl:6
    # copies of the same input are bit-identical wherever they sit: in a full wavefront or the ragged one, whichever lane or team
    first = np.arange(N) % NT
    for name, a in (("filter mean", mf), ("filter cov", cf), ("smoothed mean", ms), ("smoothed cov", cs), ("diffusions", diff), ("loglik", ll)):
        np.testing.assert_array_equal(a, a[first], err_msg=f"{name}: copies of one trajectory differ by position")
    np.testing.assert_array_equal(mf[:, 0, :d], fx["u0s"][first])
    assert np.all(cf[:, 0] == 0.0)
    return ratios


# ------------------------------------------------------------------------------------------------------------ fixedMAP
MAP_COMBOS = [(c, f, s) for c in X.model_cases("map") for f in X.filter_families(_dim(c)) for s in X.smoother_families(_dim(c))]


def solve_map(pkg, case, filt, smoother, setenv):
    family, rhs, kind, q, diffusion, dt = case
    fx = X.load(X.model_name(case))
    for k, v in {**X.FILTER_ENV[filt], **X.SMOOTH_ENV[smoother]}.items():
        setenv(k, v)
    alg = (pkg.EK1 if kind == "EK1" else pkg.EK0)(order=q, diffusionmodel=diffusion, smooth=True)
    return fx, pkg.solve(_problem(pkg, case, fx), alg, pkg.EnsembleHIP(), tstops=fx["t"], adaptive=False)


def check_map(fx, sol, case, filt, smoother):
    family, rhs, kind, q, diffusion, dt = case
    assert sol.ctx.kernel_name(0).startswith(X.filter_kernel_name(filt, rhs, q, kind == "EK1")), sol.ctx.kernel_name(0)
    assert sol.ctx.kernel_name(1) == X.smoother_kernel_name(smoother, X.MODEL_DIM[rhs], q), sol.ctx.kernel_name(1)
    return check_model(fx, sol, case, f"{filt}+{smoother}")


@pytest.mark.parametrize("case,filt,smoother", MAP_COMBOS, ids=[f"{X.model_id(c)}-{f}+{s}" for c, f, s in MAP_COMBOS])
def test_fixed_map_against_extended_precision(pkg, case, filt, smoother, monkeypatch):
    """The on-line MAP update of the global diffusion (ek_math.h, fixed_diffusion == 2) and the postamble, on every pair of
    filter and smoother family the launchers can select for the case's state dimension."""
    fx, sol = solve_map(pkg, case, filt, smoother, monkeypatch.setenv)
    check_map(fx, sol, case, filt, smoother)


# ----------------------------------------------------------------------------------------------------------- MV models
MV_COMBOS = [(c, f) for c in X.model_cases("mv") for f in ("lane_lag", "lane")]


def solve_mv(pkg, case, filt, setenv):
    family, rhs, kind, q, diffusion, dt = case
    fx = X.load(X.model_name(case))
    setenv("ODEF_FILTER_LAG_MAX_N", LAG_ENV[filt])
    return fx, pkg.solve(_problem(pkg, case, fx), pkg.EK0(order=q, diffusionmodel=diffusion, smooth=True), pkg.EnsembleHIP(), tstops=fx["t"],
                         adaptive=False)


def check_mv(fx, sol, case, filt):
    family, rhs, kind, q, diffusion, dt = case
    lag = "true" if filt == "lane_lag" else "false"
    assert sol.ctx.kernel_name(0) == f"odef::ek_filter_fixed_mv_kernel<odef::{X.MODEL_RHS_STRUCT[rhs]}, {q}, true, {lag}>", sol.ctx.kernel_name(0)
    assert sol.ctx.kernel_name(1) == f"odef::rts_smooth_mv_kernel<{X.MODEL_DIM[rhs]}, {q}>", sol.ctx.kernel_name(1)
    return check_model(fx, sol, case, filt)


@pytest.mark.parametrize("case,filt", MV_COMBOS, ids=[f"{X.model_id(c)}-{f}" for c, f in MV_COMBOS])
def test_mv_models_against_extended_precision(pkg, case, filt, monkeypatch):
    """:dynamicMV / :fixedMV: the MV lane filter with and without lagged record stores (d diffusions per record), the postamble of
    :fixedMV and rts_smooth_mv_kernel."""
    fx, sol = solve_mv(pkg, case, filt, monkeypatch.setenv)
    check_mv(fx, sol, case, filt)


# ---------------------------------------------------------------------------------------------------------------- IEKS
def _filter_families(case):
    return [f for f in ("rows", "lane_lag", "lane") if f != "rows" or _dim(case) <= 16]


IEKS_COMBOS = [(c, f) for c in X.model_cases("ieks") for f in _filter_families(c)]


def solve_ieks(pkg, case, filt, monkeypatch):
    family, rhs, kind, q, diffusion, dt = case
    fx = X.load(X.model_name(case))
    TI._family_env(monkeypatch, filt)
    return fx, pkg.solve_ieks(_problem(pkg, case, fx), pkg.IEKS(order=q, diffusionmodel=diffusion), pkg.EnsembleHIP(), tstops=fx["t"],
                              adaptive=False, iterations=int(fx["iterations"]))


def check_ieks(fx, sol, case, filt):
    TI._check_kernel(sol, filt)
    assert X.MODEL_RHS_STRUCT[case[1]] in sol.ctx.kernel_name(0)
    return check_model(fx, sol, case, filt)


@pytest.mark.parametrize("case,filt", IEKS_COMBOS, ids=[f"{X.model_id(c)}-{f}" for c, f in IEKS_COMBOS])
def test_ieks_third_iteration_against_extended_precision(pkg, case, filt, monkeypatch):
    """Three iterations of solve_ieks on ek_filter_rows_ieks_kernel and ek_filter_fixed_ieks_kernel (lagged and plain stores), the
    linearisation points handed from the smoother to the next filter on the device; one case per diffusion model."""
    fx, sol = solve_ieks(pkg, case, filt, monkeypatch)
    check_ieks(fx, sol, case, filt)
    sol.ctx.close()


# -------------------------------------------------------------------------------------------------------------- forced
FORCED_COMBOS = [(c, f) for c in X.model_cases("forced") for f in _filter_families(c)]


def solve_forced(pkg, case, filt, monkeypatch):
    family, rhs, kind, q, diffusion, dt = case
    fx = X.load(X.model_name(case))
    TT._family_env(monkeypatch, filt)
    alg = (pkg.EK1 if kind == "EK1" else pkg.EK0)(order=q, smooth=True)
    return fx, pkg.solve(_problem(pkg, case, fx), alg, pkg.EnsembleHIP(), tstops=fx["t"], adaptive=False)


def check_forced(fx, sol, case, filt):
    TT._check_family(sol, filt)
    assert "RhsForced" in sol.ctx.kernel_name(0)
    return check_model(fx, sol, case, filt)


@pytest.mark.parametrize("case,filt", FORCED_COMBOS, ids=[f"{X.model_id(c)}-{f}" for c, f in FORCED_COMBOS])
def test_forced_field_against_extended_precision(pkg, case, filt, monkeypatch):
    """f(u, p, t) from t0 = 0.25: every derivative block of every record, and blocks 1 ... q of the initial record on their own
    (the Taylor-mode time jet), on the row-team kernel and the lane kernel with lagged and plain stores."""
    fx, sol = solve_forced(pkg, case, filt, monkeypatch)
    check_forced(fx, sol, case, filt)


def test_every_forced_family_is_in_the_lists():
    assert len(MAP_COMBOS) == 6 + 6 + 6  # D = 6, 12, 12: 2 filters x 3 smoothers each
    assert len(MV_COMBOS) == 2 * len(X.model_cases("mv")) and len(IEKS_COMBOS) == 9 and len(FORCED_COMBOS) == 9
