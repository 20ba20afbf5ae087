"""Time-dependent vector fields f(u, p, t) on the device: the compiled-in field `forced` and run-time compiled
`has_time` structs on the lane and row-team kernels, against the reference for time-dependent fields (tests/_time_reference.py,
pinned by tests/test_time_reference.py).  Needs a real MI355X.

Bars: those of test_mv_parity at q <= 3, the project's established distance between two fp64 evaluations of one step.
Fixed grids: means rtol 1e-10, covariances P.cov_err < 1e-6, log-likelihood 1e-9.  Adaptive: identical (naccept, nreject),
sol.t 1e-8, means 1e-6, covariances 1e-4."""
import numpy as np
import pytest

import _ieks_reference as ier
import _mv_reference as mvr
import _parity as P
import _time_reference as tr
import odefilter_oracle as orc

pytestmark = pytest.mark.gpu

N = 70
SCALE = 1e-2
TSPAN = (0.25, 1.25)
DT = 2.0**-6
ADAPT = dict(adaptive=True, abstol=1e-6, reltol=1e-4, dt=1e-2)
# kernel family -> (ODEF_FILTER_ROWS_MAX_N, ODEF_FILTER_LAG_MAX_N, name fragment, last template argument of the lane kernel)
FAMILIES = {"rows": (None, None, "ek_filter_rows", None), "lane_lag": ("0", None, "ek_filter_fixed_kernel", "true>"),
            "lane": ("0", "0", "ek_filter_fixed_kernel", "false>")}

FORCED_SRC = """
struct NAME {
  static constexpr int d = 2, np = 3;
  static constexpr bool has_time = true;
  template <class T>
  __device__ static void f(const T (&u)[2], const double* p, T t, T (&du)[2]) {
    du[0] = p[0] * u[0] + p[1] * t;
    du[1] = p[2] * t * u[1];
  }
JAC
};
"""
FORCED_JAC = """  __device__ static void jac(const double (&u)[2], const double* p, double t, double (&J)[2][2]) {
    J[0][0] = p[0]; J[0][1] = 0.0; J[1][0] = 0.0; J[1][1] = p[2] * t;
  }"""
L96_SRC = """
struct TimeL96 {
  static constexpr int d = 5, np = 2;
  static constexpr bool has_time = true;
  template <class T>
  __device__ static void f(const T (&u)[5], const double* p, T t, T (&du)[5]) {
    for (int i = 0; i < 5; ++i) du[i] = (u[(i + 1) % 5] - u[(i + 3) % 5]) * u[(i + 4) % 5] - u[i] + (p[0] + p[1] * t);
  }
  __device__ static void jac(const double (&u)[5], const double* /*p*/, double /*t*/, double (&J)[5][5]) {
    for (int a = 0; a < 5; ++a)
      for (int b = 0; b < 5; ++b) J[a][b] = 0.0;
    for (int i = 0; i < 5; ++i) {
      const int ip = (i + 1) % 5, im2 = (i + 3) % 5, im1 = (i + 4) % 5;
      J[i][ip] += u[im1];
      J[i][im2] -= u[im1];
      J[i][im1] += u[ip] - u[im2];
      J[i][i] -= 1.0;
    }
  }
};
"""
AUG_SRC = """
struct TimeAug {  // `forced` with the time appended as a state, u2' = 1: the route an autonomous-only library leaves
  static constexpr int d = 3, np = 3;
  template <class T>
  __device__ static void f(const T (&u)[3], const double* p, T (&du)[3]) {
    du[0] = p[0] * u[0] + p[1] * u[2];
    du[1] = p[2] * u[2] * u[1];
    du[2] = 0.0 * u[2] + 1.0;
  }
  __device__ static void jac(const double (&u)[3], const double* p, double (&J)[3][3]) {
    J[0][0] = p[0]; J[0][1] = 0.0;         J[0][2] = p[1];
    J[1][0] = 0.0;  J[1][1] = p[2] * u[2]; J[1][2] = p[2] * u[1];
    J[2][0] = 0.0;  J[2][1] = 0.0;         J[2][2] = 0.0;
  }
};
"""


def _family_env(monkeypatch, family):
    rows, lag = FAMILIES[family][:2]
    for var, v in (("ODEF_FILTER_ROWS_MAX_N", rows), ("ODEF_FILTER_LAG_MAX_N", lag)):
        if v is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, v)


def _check_family(sol, family):
    name = sol.ctx.kernel_name(0)
    assert FAMILIES[family][2] in name, name
    if FAMILIES[family][3]:
        assert name.endswith(FAMILIES[family][3]), name


def _solve(pkg, field, alg, **kw):
    vf = tr.forced()
    ens = pkg.EnsembleProblem(pkg.ODEProblem(field, vf.u0, TSPAN, vf.p), perturb_scale=SCALE)
    return pkg.solve(ens, alg, pkg.EnsembleHIP(), trajectories=N, **kw)


_REFS = {}


def _ref(kind, q, i, adaptive, smooth=True):
    """The reference solve of trajectory i, computed once and shared."""
    key = (kind, q, i, adaptive)
    if key not in _REFS:
        vf = tr.forced()
        u0 = orc.ensemble_u0(vf.u0, N, SCALE)[i]
        kw = ADAPT if adaptive else dict(dt=DT)
        _REFS[key] = orc.solve(vf, orc.Alg(kind, q, "dynamic", True), u0=u0, tspan=TSPAN, **kw)
    return _REFS[key]


def _check_fixed(sol, ref, i, d=2):
    n = len(ref.t)
    assert int(sol.nsaved[i]) == n
    np.testing.assert_allclose(sol.x_filt_mean()[i, :n, :d], ref.means(smoothed=False)[:, :d], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(sol.u[i, :n], ref.u, rtol=1e-10, atol=1e-12)
    assert P.cov_err(sol.x_filt_cov()[i, :n], ref.covs(smoothed=False)) < 1e-6
    assert P.cov_err(sol.x_smooth_cov()[i, :n], ref.covs(smoothed=True)) < 1e-6
    assert abs(sol.log_likelihood[i] - ref.log_likelihood) <= 1e-9 * abs(ref.log_likelihood)


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("q", [1, 2, 3])
@pytest.mark.parametrize("kind", ["EK0", "EK1"])
def test_fixed_grid_parity(pkg, monkeypatch, kind, q, family):
    _family_env(monkeypatch, family)
    sol = _solve(pkg, "forced", getattr(pkg, kind)(order=q), dt=DT, adaptive=False)
    assert sol.retcode == ["Success"] * N
    _check_family(sol, family)
    assert "RhsForced" in sol.ctx.kernel_name(0)
    np.testing.assert_array_equal(sol.t, orc.fixed_time_grid(*TSPAN, DT))
    for i in (0, N - 1):
        _check_fixed(sol, _ref(kind, q, i, False), i)


@pytest.mark.parametrize("family", ["rows", "lane"])
@pytest.mark.parametrize("q", [1, 2, 3])
@pytest.mark.parametrize("kind", ["EK0", "EK1"])
def test_adaptive_parity(pkg, monkeypatch, kind, q, family):
    _family_env(monkeypatch, family)
    sol = _solve(pkg, "forced", getattr(pkg, kind)(order=q), **ADAPT)
    assert sol.retcode == ["Success"] * N
    assert ("ek_filter_rows_adaptive_kernel" if family == "rows" else "ek_filter_adaptive_kernel") in sol.ctx.kernel_name(0)
    for i in (0, N - 1):
        ref = _ref(kind, q, i, True)
        n = len(ref.t)
        assert (int(sol.destats.naccept[i]), int(sol.destats.nreject[i])) == (ref.naccept, ref.nreject)
        assert int(sol.nsaved[i]) == n
        np.testing.assert_allclose(sol.t[i, :n], ref.t, rtol=1e-8)
        np.testing.assert_allclose(sol.x_filt_mean()[i, :n, :2], ref.means(smoothed=False)[:, :2], rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(sol.u[i, :n], ref.u, rtol=1e-6, atol=1e-12)
        assert P.cov_err(sol.x_filt_cov()[i, :n], ref.covs(smoothed=False)) < 1e-4
        assert P.cov_err(sol.x_smooth_cov()[i, :n], ref.covs(smoothed=True)) < 1e-4


def test_smoother_dense_output_and_sampling_read_the_records(pkg):
    """The passes behind the filter share the autonomous kernels: this guards the records they read."""
    q = 3
    sol = _solve(pkg, "forced", pkg.EK1(order=q), dt=DT, adaptive=False)
    consts = orc.make_consts(2, q)
    tq = np.array([0.26, 0.5, 0.9, 1.249])
    qm, qc = sol(tq)
    n_s, seed = 3, 17
    st = sol.sample_states(n_s, seed)
    for i in (0, N - 1):
        ref = _ref("EK1", q, i, False)
        n = len(ref.t)
        np.testing.assert_allclose(sol.x_smooth_mean()[i, :n, :2], ref.means(smoothed=True)[:, :2], rtol=1e-10, atol=1e-12)
        assert P.cov_err(sol.x_smooth_cov()[i, :n], ref.covs(smoothed=True)) < 1e-6
        for k, tv in enumerate(tq):
            g = orc.dense_output(ref, consts, float(tv), smoothed=True)
            np.testing.assert_allclose(qm[i, k, :2], g.mu[:2], rtol=1e-9, atol=1e-12)
            assert P.cov_err(qc[i, k][None], g.cov()[None]) < 1e-4
        cap, D = st.shape[1], st.shape[2]  # the device's noise stream and square root (tests/test_gpu_parity.py::test_posterior_sampling)
        want = orc.sample_states(ref, consts, n_s, sqrt="cholesky", normal=lambda j, slot, k: orc.sample_normal(seed, i, j, slot, k, n_s, cap, D))
        scale = np.abs(want).max(axis=(0, 2))[None, :, None]
        err = (np.abs(st[i, :n] - want) / scale).max(axis=(0, 2))
        assert err[:2].max() < 1e-8 and err.max() < 1e-2, err


@pytest.mark.parametrize("family", ["rows", "lane"])
def test_final_state_mode_is_the_last_record(pkg, monkeypatch, family):
    _family_env(monkeypatch, family)
    every = _solve(pkg, "forced", pkg.EK1(order=3, smooth=False), dt=DT, adaptive=False)
    last = _solve(pkg, "forced", pkg.EK1(order=3, smooth=False), dt=DT, adaptive=False, save_everystep=False)
    assert "false" in last.ctx.kernel_name(0).split("RhsForced")[1]
    np.testing.assert_array_equal(last.x_filt_mean()[:, -1], every.x_filt_mean()[:, -1])
    np.testing.assert_array_equal(last.x_filt_cov()[:, -1], every.x_filt_cov()[:, -1])
    np.testing.assert_array_equal(last.log_likelihood, every.log_likelihood)


def test_ieks_three_iterations(pkg):
    vf, q = tr.forced(), 2
    ens = pkg.EnsembleProblem(pkg.ODEProblem("forced", vf.u0, TSPAN, vf.p), perturb_scale=SCALE)
    sol = pkg.solve_ieks(ens, pkg.IEKS(order=q), pkg.EnsembleHIP(), trajectories=N, dt=DT, adaptive=False, iterations=3)
    assert sol.retcode == ["Success"] * N and "ieks" in sol.ctx.kernel_name(0) and "RhsForced" in sol.ctx.kernel_name(0)
    grid = orc.fixed_time_grid(*TSPAN, DT)
    u0s = orc.ensemble_u0(vf.u0, N, SCALE)
    for i in (0, N - 1):
        r = ier.solve_ieks(vf, q, "dynamic", grid, 3, u0=u0s[i])
        rel = lambda a, b: float(np.nanmax(np.abs(a - b)) / np.nanmax(np.abs(b)))  # noqa: E731
        assert rel(sol.x_smooth_mean()[i], r.means(smoothed=True)) < 1e-9
        assert rel(sol.x_filt_mean()[i], r.means(smoothed=False)) < 1e-9
        assert rel(sol.x_smooth_cov()[i], r.covs(smoothed=True)) < 1e-6
        assert abs(sol.log_likelihood[i] - r.log_likelihood) <= 1e-7 * abs(r.log_likelihood)


def test_dynamic_mv_ek0(pkg):
    vf, q = tr.forced(), 3
    sol = _solve(pkg, "forced", pkg.EK0(order=q, diffusionmodel="dynamicMV"), dt=DT, adaptive=False)
    assert sol.retcode == ["Success"] * N and "ek_filter_fixed_mv_kernel" in sol.ctx.kernel_name(0)
    u0s = orc.ensemble_u0(vf.u0, N, SCALE)
    for i in (0, N - 1):
        ref = mvr.solve(vf, "dynamicMV", q, u0=u0s[i], tspan=TSPAN, dt=DT)
        n = len(ref.t)
        np.testing.assert_allclose(sol.x_filt_mean()[i, :n, :2], ref.means(smoothed=False)[:, :2], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(sol.u[i, :n], ref.u, rtol=1e-10, atol=1e-12)
        d = np.array(ref.diffusions)
        assert float(np.abs(sol.diffusions[i, : n - 1] - d).max() / np.abs(d).max()) < 1e-8
        assert P.cov_err(sol.x_filt_cov()[i, :n], ref.covs(smoothed=False)) < 1e-6
        assert P.cov_err(sol.x_smooth_cov()[i, :n], ref.covs(smoothed=True)) < 1e-6
        np.testing.assert_allclose(sol.log_likelihood[i], ref.log_likelihood, rtol=1e-9)


@pytest.fixture(scope="module")
def jit_fields(pkg):
    pkg.compile_rhs("TimeForced", FORCED_SRC.replace("NAME", "TimeForced").replace("JAC", FORCED_JAC), 2, 3)
    pkg.compile_rhs("TimeForcedFwd", FORCED_SRC.replace("NAME", "TimeForcedFwd").replace("JAC", ""), 2, 3)
    return ("TimeForced", "TimeForcedFwd")


def test_run_time_field_equals_the_compiled_in_one(pkg, jit_fields):
    for kw in (dict(dt=DT, adaptive=False), ADAPT):
        a = _solve(pkg, "forced", pkg.EK1(order=3), **kw)
        b = _solve(pkg, jit_fields[0], pkg.EK1(order=3), **kw)
        assert "TimeForced" in b.ctx.kernel_name(0) and "ek_filter_rows" in b.ctx.kernel_name(0)
        np.testing.assert_array_equal(a.nsaved, b.nsaved)
        np.testing.assert_allclose(b.x_filt_mean(), a.x_filt_mean(), rtol=1e-13, atol=1e-300)
        np.testing.assert_allclose(b.x_smooth_mean(), a.x_smooth_mean(), rtol=1e-13, atol=1e-300)


def test_run_time_field_without_jac_uses_forward_mode(pkg, jit_fields):
    sol = _solve(pkg, jit_fields[1], pkg.EK1(order=2), dt=DT, adaptive=False)
    assert sol.retcode == ["Success"] * N and (sol.destats.njacs == len(sol.t) - 1).all()
    for i in (0, N - 1):
        _check_fixed(sol, _ref("EK1", 2, i, False), i)


def test_run_time_field_no_compiled_in_kernel_covers(pkg):
    """d = 5, q = 2 (D = 15): Lorenz-96 with five variables and the forcing F + a t, on the row-team kernels."""
    vf, q = tr.lorenz96_forced(5), 2
    pkg.compile_rhs("TimeL96", L96_SRC, 5, 2)
    ens = pkg.EnsembleProblem(pkg.ODEProblem("TimeL96", vf.u0, vf.tspan, vf.p), perturb_scale=SCALE)
    sol = pkg.solve(ens, pkg.EK1(order=q), pkg.EnsembleHIP(), trajectories=N, dt=2.0**-7, adaptive=False)
    assert sol.retcode == ["Success"] * N and "ek_filter_rows_kernel<odef::TimeL96" in sol.ctx.kernel_name(0)
    u0s = orc.ensemble_u0(vf.u0, N, SCALE)
    for i in (0, N - 1):
        ref = orc.solve(vf, orc.EK1(order=q, smooth=True), u0=u0s[i], tspan=vf.tspan, dt=2.0**-7)
        _check_fixed(sol, ref, i, d=5)


def test_against_augmentation(pkg):
    """`forced` EK1(3) against the d = 3 run-time field with u_2 = t appended.  The posteriors differ ON PURPOSE -- the augmented
    filter carries uncertainty about t and measures u_2' = 1 along with the rest -- so the u_0, u_1 means agree to the solver's
    error (5 x the l-infinity of sol.errors), not to rounding."""
    vf = tr.forced()
    pkg.compile_rhs("TimeAug", AUG_SRC, 3, 3)
    nat = _solve(pkg, "forced", pkg.EK1(order=3), dt=DT, adaptive=False)
    u0s = np.concatenate([orc.ensemble_u0(vf.u0, N, SCALE), np.full((N, 1), TSPAN[0])], axis=1)
    ens = pkg.EnsembleProblem(pkg.ODEProblem("TimeAug", u0s[0], TSPAN, vf.p), u0s=u0s)
    aug = pkg.solve(ens, pkg.EK1(order=3), pkg.EnsembleHIP(), dt=DT, adaptive=False)
    assert aug.retcode == ["Success"] * N
    # (the augmented filter ESTIMATES t: its u_2 is the grid only to the size of its own posterior error)
    np.testing.assert_allclose(aug.u[:, :, 2], np.broadcast_to(nat.t, (N, len(nat.t))), rtol=1e-6)
    bound = 5.0 * nat.errors["l∞"]
    diff = np.abs(aug.u[:, :, :2] - nat.u).max(axis=(1, 2))
    assert (diff <= bound).all(), (diff.max(), bound.min())
    assert diff.max() > 1e-13  # not the same posterior


@pytest.mark.parametrize("q", [1, 2, 3])
@pytest.mark.parametrize("kind", ["EK0", "EK1"])
def test_convergence_orders_from_device_side_errors(pkg, kind, q):
    """sol.errors["final"] and ["l2"] of `forced` over dt = 2^-4 .. 2^-6 give q + 1 within the reference's TESTTOL = 0.2
    (test/convergence.jl); the analytic solution needs t0, which the error kernels take from the first record's time.
    The errors are those of the FILTER records (smooth=False): q + 1 is the filter's global order, and the oracle gives it for
    `l2` too (EK0 1.99 / 2.95 / 3.90, EK1 2.08 / 3.02 / 4.07 at q = 1, 2, 3).  The smoothed means converge FASTER on this field in
    the oracle itself (`l2` of EK1: 3.47 at q = 2, 4.31 at q = 3, towards q + 3/2), so an order of q + 1 is not what a correct
    smoothed solve shows; `final` is the same number either way, the last record is not smoothed."""
    vf = tr.forced()
    prob = pkg.ODEProblem("forced", vf.u0, vf.tspan, vf.p)
    errs = {"final": [], "l2": []}
    for dt in (2.0**-4, 2.0**-5, 2.0**-6):
        sol = pkg.solve(prob, getattr(pkg, kind)(order=q, smooth=False), pkg.EnsembleHIP(), dt=dt, adaptive=False)
        np.testing.assert_allclose(sol.u_analytic[0], tr.forced_analytic(vf.u0, vf.p, vf.tspan[0], sol.t), rtol=1e-13)
        for k in errs:
            errs[k].append(float(sol.errors[k][0]))
    est = {k: float(np.mean(np.log2(np.array(v[:-1]) / np.array(v[1:])))) for k, v in errs.items()}
    print(f"{kind}({q}): errors {errs}  estimated orders {est}")
    assert abs(est["final"] - (q + 1)) <= 0.2
    assert abs(est["l2"] - (q + 1)) <= 0.2
