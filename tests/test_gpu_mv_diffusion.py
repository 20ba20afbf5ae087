"""The diagonal diffusion models :dynamicMV / :fixedMV of EK0 on the device (src/diffusions.jl:83-153), against the numpy
restatement tests/_mv_reference.py (itself anchored to the oracle by tests/test_mv_reference.py).  Needs a real MI355X."""
import numpy as np
import pytest

import _mv_reference as mvr
import _parity as P
import odefilter_oracle as orc

pytestmark = pytest.mark.gpu

MODELS = ["dynamicMV", "fixedMV"]


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.nanmax(np.abs(a - b)) / (np.nanmax(np.abs(b)) + 1e-300))


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("field,q,N", [("fhn", 1, 70), ("lorenz63", 3, 70), ("lotka_volterra", 5, 70), ("lorenz63", 5, 1000),
                                       ("fhn", 3, 1000)])
def test_mv_parity(pkg, field, q, N, model, adaptive):
    """Filter, smoother, sol(t) and sample_states against the restatement; N = 70 is an ensemble the scalar models give to the
    row-team kernels, 1 000 is not a multiple of 64.  The MV kernels are the ones launched."""
    from odefilters_jl_amd import host

    vf = orc.vector_field(field)
    t1 = 0.25
    ens = pkg.EnsembleProblem(pkg.ODEProblem(field, vf.u0, (0.0, t1), vf.p), perturb_scale=1e-2)
    kw = dict(adaptive=True, dt=2.0**-8) if adaptive else dict(adaptive=False, dt=2.0**-6)
    sol = pkg.solve(ens, pkg.EK0(order=q, diffusionmodel=model), pkg.EnsembleHIP(), trajectories=N, **kw)
    assert sol.retcode == ["Success"] * N
    k0, k1 = sol.ctx.kernel_name(0), sol.ctx.kernel_name(1)
    assert ("ek_filter_adaptive_mv_kernel" if adaptive else "ek_filter_fixed_mv_kernel") in k0 and "rts_smooth_mv_kernel" in k1
    assert sol.ctx.field_bytes(host.F_DIFFUSION) == 8 * vf.d * sol.ctx.n_save * N
    d, D = vf.d, vf.d * (q + 1)
    consts = orc.make_consts(d, q)
    u0s = orc.ensemble_u0(vf.u0, N, 1e-2)
    tq = np.array([0.01, 0.1, 0.2, 0.249])
    qm, qc = sol(tq)
    n_s, seed = 3, 17
    st = None if adaptive else sol.sample_states(n_s, seed)
    for i in (0, N - 1):
        ref = mvr.solve(vf, model, q, u0=u0s[i], tspan=(0.0, t1), **kw)
        n = len(ref.t)
        assert int(sol.nsaved[i]) == n
        # sigma_a = z_a^2 / (H Q H')_11 or / S_11 rests on ONE component of the residual z, a cancellation (exact Taylor
        # initialisation: z ~ 0 at the first step; tests/_parity.py on the highest derivatives).  At order 5 two fp64 evaluations
        # of the same step agree on it to ~1e-5 only, and under adaptive steps that moves the step sizes the controller picks
        # (same accept / reject sequence, times ~1e-5 apart): the bars below are rounding noise at q <= 3 and that noise at q = 5.
        hi = q >= 5
        if adaptive:
            assert (int(sol.destats.naccept[i]), int(sol.destats.nreject[i])) == (ref.naccept, ref.nreject)
            np.testing.assert_allclose(sol.t[i, :n], ref.t, rtol=1e-4 if hi else 1e-8)
        rt = (1e-3 if hi else 1e-6) if adaptive else (1e-8 if hi else 1e-10)
        np.testing.assert_allclose(sol.x_filt_mean()[i, :n, :d], ref.means(smoothed=False)[:, :d], rtol=rt, atol=1e-12)
        np.testing.assert_allclose(sol.u[i, :n], ref.u, rtol=rt, atol=1e-12)
        rd = 1e-3 if hi else (1e-5 if adaptive else 1e-8)
        rc = (1e-2 if adaptive else 1e-3) if hi else (1e-4 if adaptive else 1e-6)
        assert _rel(sol.diffusions[i, : n - 1], np.array(ref.diffusions)) < rd
        assert P.cov_err(sol.x_filt_cov()[i, :n], ref.covs(smoothed=False)) < rc
        assert P.cov_err(sol.x_smooth_cov()[i, :n], ref.covs(smoothed=True)) < rc
        if model == "fixedMV":
            assert np.isnan(sol.log_likelihood[i])
        else:
            np.testing.assert_allclose(sol.log_likelihood[i], ref.log_likelihood, rtol=1e-5 if (adaptive or hi) else 1e-9)
        for k, tv in enumerate(tq):
            g = mvr.dense_output(ref, consts, float(tv), smoothed=True)
            np.testing.assert_allclose(qm[i, k, :d], g.mu[:d], rtol=rt * 10, atol=1e-12)
            assert P.cov_err(qc[i, k][None], g.cov()[None]) < max(rc, 1e-4)
        if not adaptive:
            want = mvr.sample_states(ref, consts, n_s, seed=seed, traj=i, n_save=st.shape[1])
            scale = np.abs(want).max(axis=(0, 2))[None, :, None]
            err = (np.abs(st[i, :n] - want) / scale).max(axis=(0, 2))
            assert err[:d].max() < (1e-6 if hi else 1e-8) and err.max() < 1e-2, err
    assert st is None or st.shape == (N, sol.ctx.n_save, D, n_s)


LOGISTIC = """
struct MvLogistic {
  static constexpr int d = 1, np = 1;
  template <class T>
  __device__ static void f(const T (&u)[1], const double* p, T (&du)[1]) { du[0] = p[0] * u[0] * (1.0 - u[0]); }
};
"""
LINEAR1 = """
struct MvLinear1 {
  static constexpr int d = 1, np = 1;
  template <class T>
  __device__ static void f(const T (&u)[1], const double* p, T (&du)[1]) { du[0] = p[0] * u[0]; }
};
"""


@pytest.fixture(scope="module")
def d1_fields(pkg):
    pkg.compile_rhs("MvLogistic", LOGISTIC, 1, 1)
    pkg.compile_rhs("MvLinear1", LINEAR1, 1, 1)
    return ("MvLogistic", "MvLinear1")


@pytest.mark.parametrize("model", MODELS)
def test_mv_identities_on_device(pkg, d1_fields, model, monkeypatch):
    """d = 1: the MV model is the scalar one (run-time compiled logistic field, fixed grid and adaptive).  A decoupled field:
    the d = 2 LINEAR solve is two d = 1 solves side by side, with zero cross-component covariance.  The scalar solves are put
    on the kernel family of the MV ones (lane filter, row-team smoother), so that the identities compare the models alone."""
    monkeypatch.setenv("ODEF_FILTER_ROWS_MAX_N", "0")
    monkeypatch.setenv("ODEF_SMOOTH_ROWS_MAX_N", "0")
    monkeypatch.setenv("ODEF_SMOOTH_LANE_MIN_N", str(1 << 40))
    scalar = {"dynamicMV": "dynamic", "fixedMV": "fixed"}[model]
    logi, lin1 = d1_fields
    for adaptive in (False, True):
        kw = dict(adaptive=True, dt=1e-2, abstol=1e-7, reltol=1e-5) if adaptive else dict(adaptive=False, dt=2.0**-5)
        sols = []
        for m in (model, scalar):
            ens = pkg.EnsembleProblem(pkg.ODEProblem(logi, np.array([0.1]), (0.0, 1.0), np.array([3.0])), perturb_scale=1e-3)
            sols.append(pkg.solve(ens, pkg.EK0(order=3, diffusionmodel=m), pkg.EnsembleHIP(), trajectories=5, **kw))
        a, b = sols
        assert "_mv_" in a.ctx.kernel_name(0) and "_mv_" not in b.ctx.kernel_name(0)
        np.testing.assert_array_equal(a.nsaved, b.nsaved)
        # fixed grid: rounding level.  Adaptive: the two models' calibrations differ in their last bits (z^2 / W against
        # |L^-1 z|^2), the controller turns that into step sizes a few ulp apart, and the top derivative block of the state
        # amplifies those (tests/_parity.py): same step sequence, agreement to 1e-5 of the state's magnitude
        tol = 1e-5 if adaptive else 1e-9
        assert _rel(a.x_filt_mean(), b.x_filt_mean()) < tol and _rel(a.x_smooth_mean(), b.x_smooth_mean()) < tol
        assert _rel(a.x_filt_cov(), b.x_filt_cov()) < tol and _rel(a.x_smooth_cov(), b.x_smooth_cov()) < tol
        assert _rel(a.diffusions[..., 0], b.diffusions) < tol
        if model == "dynamicMV":
            assert _rel(a.log_likelihood, b.log_likelihood) < tol
    vf = orc.vector_field("linear")
    q = 2
    ens = pkg.EnsembleProblem(pkg.ODEProblem("linear", vf.u0, (0.0, 1.0), vf.p), u0s=np.tile(vf.u0, (4, 1)))
    mv = pkg.solve(ens, pkg.EK0(order=q, diffusionmodel=model), pkg.EnsembleHIP(), dt=2.0**-4, adaptive=False)
    ll = 0.0
    for a in range(2):
        ens1 = pkg.EnsembleProblem(pkg.ODEProblem(lin1, vf.u0[a : a + 1], (0.0, 1.0), vf.p[a : a + 1]), u0s=np.full((4, 1), vf.u0[a]))
        one = pkg.solve(ens1, pkg.EK0(order=q, diffusionmodel=scalar), pkg.EnsembleHIP(), dt=2.0**-4, adaptive=False)
        idx = np.arange(q + 1) * 2 + a
        assert _rel(mv.x_filt_mean()[..., idx], one.x_filt_mean()) < 1e-9
        assert _rel(mv.x_smooth_mean()[..., idx], one.x_smooth_mean()) < 1e-9
        assert _rel(mv.x_filt_cov()[..., idx[:, None], idx[None, :]], one.x_filt_cov()) < 1e-9
        assert _rel(mv.x_smooth_cov()[..., idx[:, None], idx[None, :]], one.x_smooth_cov()) < 1e-9
        assert _rel(mv.diffusions[..., a], one.diffusions) < 1e-9
        ll = ll + one.log_likelihood
    comp = np.arange(2 * (q + 1)) % 2
    cross = comp[:, None] != comp[None, :]
    assert np.all(mv.x_filt_cov()[..., cross] == 0.0) and np.all(mv.x_smooth_cov()[..., cross] == 0.0)
    if model == "dynamicMV":
        assert _rel(mv.log_likelihood, ll) < 1e-9


def _fhn_rk4(u0, p, grid, sub=10):
    a, b, c = p

    def f(x, y):
        return c * (x - x**3 / 3.0 + y), -(x - a - b * y) / c

    out = np.empty((len(grid), 2))
    x, y = float(u0[0]), float(u0[1])
    out[0] = x, y
    for n in range(len(grid) - 1):
        h = (grid[n + 1] - grid[n]) / sub
        for _ in range(sub):
            k1 = f(x, y)
            k2 = f(x + 0.5 * h * k1[0], y + 0.5 * h * k1[1])
            k3 = f(x + 0.5 * h * k2[0], y + 0.5 * h * k2[1])
            k4 = f(x + h * k3[0], y + h * k3[1])
            x += h / 6.0 * (k1[0] + 2 * k2[0] + 2 * k3[0] + k4[0])
            y += h / 6.0 * (k1[1] + 2 * k2[1] + 2 * k3[1] + k4[1])
        out[n + 1] = x, y
    return out


def test_reference_diffusions_check(pkg):
    """test/diffusions.jl:22-30 of the reference: FHN, EK0(order=3) with :dynamicMV / :fixedMV (and :dynamic as the control),
    adaptive=false, dt=1e-4, `sol.u ≈ true_sol.(sol.t)` -- Julia's ≈ on the vector of states: norm(diff) <= sqrt(eps) max(norms).
    The true solution: RK4 at dt = 1e-5 on the same grid points (error far below 1e-12)."""
    vf = orc.vector_field("fhn")
    prob = pkg.ODEProblem("fhn", vf.u0, (0.0, 1.0), vf.p)
    truth = None
    for model in ("dynamicMV", "fixedMV", "dynamic"):
        sol = pkg.solve(prob, pkg.EK0(order=3, diffusionmodel=model), dt=1e-4, adaptive=False)
        assert sol.retcode == ["Success"]
        if truth is None:
            truth = _fhn_rk4(vf.u0, vf.p, sol.t)
        u = sol.u[0]
        assert u.shape == truth.shape
        assert np.linalg.norm(u - truth) <= np.sqrt(np.finfo(float).eps) * max(np.linalg.norm(u), np.linalg.norm(truth)), model


def test_mv_refusals(pkg):
    from odefilters_jl_amd import host

    vf = orc.vector_field("lorenz63")
    prob = pkg.ODEProblem("lorenz63", vf.u0, (0.0, 0.1), vf.p)
    for model in MODELS:
        with pytest.raises(pkg.OdefError, match="require EK0"):
            pkg.solve(prob, pkg.EK1(order=3, diffusionmodel=model), dt=0.01, adaptive=False)
        with pytest.raises(pkg.OdefError, match="require EK0"):  # the C ABI refuses it too
            host.Context("lorenz63", 3, host.EK1_ID, 4, diffusion=model)
        with pytest.raises(pkg.OdefError, match="lane kernels only"):
            host.Context("pleiades", 2, host.EK0_ID, 4, diffusion=model)
        with pytest.raises(pkg.OdefError, match="lane kernels only"):
            host.Context("lorenz96", 2, host.EK0_ID, 4, diffusion=model)
    # a run-time compiled field above state dimension 20 (the workgroup-per-trajectory kernels)
    src = """
struct MvBig12 {
  static constexpr int d = 12, np = 0;
  template <class T>
  __device__ static void f(const T (&u)[12], const double* p, T (&du)[12]) { for (int i = 0; i < 12; ++i) du[i] = -u[i]; }
};
"""
    pkg.compile_rhs("MvBig12", src, 12, 0)
    big = pkg.ODEProblem("MvBig12", np.ones(12), (0.0, 0.1), ())
    with pytest.raises(pkg.OdefError, match="lane kernels only"):
        pkg.solve(big, pkg.EK0(order=1, diffusionmodel="fixedMV"), dt=0.01, adaptive=False)


def test_group_two_shards_fixed_mv(pkg):
    """Two shards of one :fixedMV ensemble on this device against one context: final means (all-gather), the d-wide
    diffusion field, the rescaled covariances, bit for bit."""
    from odefilters_jl_amd import host

    vf = orc.vector_field("lorenz63")
    N = 1001
    grid = np.arange(33) * 2.0**-9
    with host.DeviceGroup("lorenz63", 3, host.EK0_ID, N, 2, device_ids=[0, 0], diffusion="fixedMV") as grp:
        assert grp.shard(0) == (0, 501) and grp.shard(1) == (501, 500)
        grp.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-2)
        grp.solve_fixed(grid)
        fin = grp.allgather(from_device=0)
        gdiff = grp.gather_field(host.F_DIFFUSION)
        gcov = grp.gather_field(host.F_COV_TRIL)
    ctx = pkg.Context("lorenz63", 3, host.EK0_ID, N, diffusion="fixedMV")
    ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-2)
    ctx.solve_fixed(grid)
    assert gdiff.shape == (33, 3, N)
    np.testing.assert_array_equal(fin, ctx.get(host.F_MEAN)[-1])
    np.testing.assert_array_equal(gdiff, ctx.get(host.F_DIFFUSION))
    np.testing.assert_array_equal(gcov, ctx.get(host.F_COV_TRIL))
    ctx.close()
