"""IEKS / solve_ieks on the device (src/ieks.jl), against the numpy restatement tests/_ieks_reference.py (itself anchored to the
oracle by tests/test_ieks_reference.py), plus the exact identities, the run-time compiled fields, the refusals and a
two-shard group.  Needs a real MI355X."""
import ctypes as C

import numpy as np
import pytest

import _ieks_reference as ier
import odefilter_oracle as orc

pytestmark = pytest.mark.gpu

# (field, order, diffusion model, dt, t1)
CASES = [("fhn", 4, "fixed", 0.1, 3.2), ("lorenz63", 3, "dynamic", 2.0**-7, 0.25), ("vanderpol", 5, "fixedMAP", 0.02, 0.64)]
# kernel family -> (ODEF_FILTER_ROWS_MAX_N, ODEF_FILTER_LAG_MAX_N, name fragment of the IEKS filter)
FAMILIES = {"rows": (None, None, "ek_filter_rows_ieks_kernel"), "lane_lag": ("0", None, "ek_filter_fixed_ieks_kernel"),
            "lane": ("0", "0", "ek_filter_fixed_ieks_kernel")}


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.nanmax(np.abs(a - b)) / (np.nanmax(np.abs(b)) + 1e-300))


def _family_env(monkeypatch, family):
    rows, lag, _ = FAMILIES[family]
    for var, v in (("ODEF_FILTER_ROWS_MAX_N", rows), ("ODEF_FILTER_LAG_MAX_N", lag)):
        if v is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, v)


def _check_kernel(sol, family):
    name = sol.ctx.kernel_name(0)
    assert FAMILIES[family][2] in name, name
    if family != "rows":
        assert name.endswith("true>" if family == "lane_lag" else "false>"), name


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("field,q,model,dt,t1", CASES)
def test_ieks_parity(pkg, monkeypatch, field, q, model, dt, t1, family):
    """Iterations 1, 2, 3 and 10 of solve_ieks against the restatement, for each kernel family (the family asserted by name);
    destats nf = njac = n_t - 1."""
    _family_env(monkeypatch, family)
    vf = orc.vector_field(field)
    N = 65
    ens = pkg.EnsembleProblem(pkg.ODEProblem(field, vf.u0, (0.0, t1), vf.p), perturb_scale=1e-2)
    grid = pkg.fixed_time_grid(0.0, t1, dt)
    u0s = orc.ensemble_u0(vf.u0, N, 1e-2)
    refs = {i: ier.solve_ieks(vf, q, model, grid, 10, u0=u0s[i], history=True) for i in (0, N - 1)}
    rt = 1e-5 if q >= 5 else 1e-9  # q = 5: Q is Hilbert-like, the higher derivatives amplify rounding (tests/_parity.py)
    for k in (1, 2, 3, 10):
        sol = pkg.solve_ieks(ens, pkg.IEKS(order=q, diffusionmodel=model), pkg.EnsembleHIP(), trajectories=N, dt=dt,
                             adaptive=False, iterations=k)
        assert sol.retcode == ["Success"] * N
        assert isinstance(sol.alg, pkg.IEKS)
        if k > 1:
            _check_kernel(sol, family)
        else:
            assert "ieks" not in sol.ctx.kernel_name(0)  # the empty field: EK1's kernel
        n = len(grid)
        assert (sol.destats.nf == n - 1).all() and (sol.destats.njacs == n - 1).all()
        for i, ref in refs.items():
            r = ref[k - 1]
            assert _rel(sol.x_smooth_mean()[i], r.means(smoothed=True)) < rt, (k, i)
            assert _rel(sol.x_filt_mean()[i], r.means(smoothed=False)) < rt, (k, i)
            assert _rel(sol.x_smooth_cov()[i], r.covs(smoothed=True)) < 1e3 * rt, (k, i)
            if model == "dynamic":
                assert abs(sol.log_likelihood[i] - r.log_likelihood) <= 1e-7 * abs(r.log_likelihood)
            else:
                assert np.isnan(sol.log_likelihood[i])
        sol.ctx.close()


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_ieks_exact_identities(pkg, monkeypatch, family):
    """An empty ODEF_F_LINEARIZE_AT is EK1, bit for bit; binding EK1's smoothed u and solving once is two solve_ieks
    iterations, bit for bit."""
    from odefilters_jl_amd import host

    _family_env(monkeypatch, family)
    vf = orc.vector_field("lorenz63")
    N, dt = 100, 2.0**-7
    ens = pkg.EnsembleProblem(pkg.ODEProblem("lorenz63", vf.u0, (0.0, 0.5), vf.p), perturb_scale=1e-2)
    kw = dict(trajectories=N, dt=dt, adaptive=False)
    ek1 = pkg.solve(ens, pkg.EK1(order=3), pkg.EnsembleHIP(), **kw)
    one = pkg.solve(ens, pkg.IEKS(order=3), pkg.EnsembleHIP(), **kw)
    assert one.ctx.kernel_name(0) == ek1.ctx.kernel_name(0)
    for f in (host.F_MEAN, host.F_COV_TRIL, host.F_DIFFUSION, host.F_LOGLIK, host.F_SMOOTH_MEAN, host.F_SMOOTH_COV_TRIL,
              host.F_NF, host.F_NJAC):
        np.testing.assert_array_equal(one.ctx.get(f), ek1.ctx.get(f))
    # odef_smooth of the IEKS context has set the field: the u rows of every smoothed save
    np.testing.assert_array_equal(one.ctx.get(host.F_LINEARIZE_AT), ek1.ctx.get(host.F_SMOOTH_MEAN)[:, :3, :])
    seeded = pkg.solve(ens, pkg.IEKS(order=3, linearize_at=ek1), pkg.EnsembleHIP(), **kw)
    _check_kernel(seeded, family)
    two = pkg.solve_ieks(ens, pkg.IEKS(order=3), pkg.EnsembleHIP(), iterations=2, **kw)
    for f in (host.F_MEAN, host.F_COV_TRIL, host.F_LOGLIK, host.F_SMOOTH_MEAN, host.F_SMOOTH_COV_TRIL):
        np.testing.assert_array_equal(seeded.ctx.get(f), two.ctx.get(f))
    assert _rel(two.u, ek1.u) > 0.0
    # linearize_at solved on another (finer) grid: its smoothed dense output on this grid is bound
    fine = pkg.solve(ens, pkg.EK1(order=3), pkg.EnsembleHIP(), trajectories=N, dt=dt / 2, adaptive=False)
    other = pkg.solve(ens, pkg.IEKS(order=3, linearize_at=fine), pkg.EnsembleHIP(), **kw)
    lin = other.ctx.get(host.F_LINEARIZE_AT)  # (the smoother has replaced the bound points by its own)
    assert np.all(np.isfinite(lin)) and _rel(other.u, two.u) < 1e-3


USER_D5 = """
struct {name} {{
  static constexpr int d = 5, np = 1;
  template <class T>
  __device__ static void f(const T (&u)[5], const double* p, T (&du)[5]) {{
    for (int i = 0; i < 5; ++i) du[i] = (u[(i + 1) % 5] - u[(i + 3) % 5]) * u[(i + 4) % 5] - u[i] + p[0];
  }}
{jac}}};
"""
USER_D5_JAC = """  __device__ static void jac(const double (&u)[5], const double* p, double (&J)[5][5]) {
    for (int i = 0; i < 5; ++i) {
      for (int k = 0; k < 5; ++k) J[i][k] = 0.0;
      J[i][(i + 1) % 5] += u[(i + 4) % 5];
      J[i][(i + 3) % 5] -= u[(i + 4) % 5];
      J[i][(i + 4) % 5] += u[(i + 1) % 5] - u[(i + 3) % 5];
      J[i][i] -= 1.0;
    }
  }
"""


def _l96_field(name, d):
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

    u0 = 8.0 + np.sin(np.arange(d))
    return orc.VectorField(name, -1, d, 1, f, jac, u0, np.array([8.0]), (0.0, 0.25))


@pytest.mark.parametrize("name,d,q,with_jac,family", [("IeksL96d5J", 5, 2, True, "lane"), ("IeksL96d5", 5, 2, False, "lane"),
                                                       ("IeksL96d4", 4, 3, False, "rows")])
def test_ieks_runtime_fields(pkg, monkeypatch, name, d, q, with_jac, family):
    """Run-time compiled Lorenz-96 fields: d = 5 on the lane kernels with f.jac and with the forward-mode Jacobian (which the
    device evaluates at the linearisation point: the documented divergence from the reference), d = 4, q = 3 (D = 16) on the
    row teams."""
    src = USER_D5.format(name=name, jac=USER_D5_JAC if with_jac else "") if d == 5 else None
    if src is None:
        src = f"""
struct {name} {{
  static constexpr int d = 4, np = 1;
  template <class T>
  __device__ static void f(const T (&u)[4], const double* p, T (&du)[4]) {{
    for (int i = 0; i < 4; ++i) du[i] = (u[(i + 1) % 4] - u[(i + 2) % 4]) * u[(i + 3) % 4] - u[i] + p[0];
  }}
}};
"""
    pkg.compile_rhs(name, src, d, 1)
    _family_env(monkeypatch, family)
    vf = _l96_field(name, d)
    N, dt, t1 = 70, 2.0**-7, 0.125
    ens = pkg.EnsembleProblem(pkg.ODEProblem(name, vf.u0, (0.0, t1), vf.p), perturb_scale=1e-2)
    grid = pkg.fixed_time_grid(0.0, t1, dt)
    sol = pkg.solve_ieks(ens, pkg.IEKS(order=q), pkg.EnsembleHIP(), trajectories=N, dt=dt, adaptive=False, iterations=3)
    assert sol.retcode == ["Success"] * N
    _check_kernel(sol, family)
    assert name in sol.ctx.kernel_name(0)
    u0s = orc.ensemble_u0(vf.u0, N, 1e-2)
    for i in (0, N - 1):
        ref = ier.solve_ieks(vf, q, "dynamic", grid, 3, u0=u0s[i])
        assert _rel(sol.x_smooth_mean()[i], ref.means(smoothed=True)) < 1e-9
        assert _rel(sol.x_filt_mean()[i], ref.means(smoothed=False)) < 1e-9


def test_ieks_refusals(pkg):
    from odefilters_jl_amd import host

    vf = orc.vector_field("lorenz63")
    for kw, msg in ((dict(smooth=False), "IEKS always smooths"), (dict(smooth=True, diffusion="dynamicMV"), "require EK0")):
        with pytest.raises(pkg.OdefError, match=msg):
            pkg.Context("lorenz63", 3, host.IEKS_ID, 64, **kw)
    with pytest.raises(pkg.OdefError, match="lane kernels only"):
        pkg.Context("pleiades", 2, host.IEKS_ID, 64, smooth=True)
    with pytest.raises(pkg.OdefError, match="lane kernels only"):
        pkg.Context("lorenz96", 2, host.IEKS_ID, 64, smooth=True)
    N = 64
    grid = np.arange(17) * 2.0**-7
    ctx = pkg.Context("lorenz63", 3, host.IEKS_ID, N, smooth=True)
    ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-2)
    ctx.solve_adaptive(0.1, dt0=1e-3, max_steps=64)  # the field is empty: EK1, allowed
    ctx.smooth()
    with pytest.raises(pkg.OdefError, match="holds no data"):  # an adaptive smoother leaves the field empty
        ctx.get(host.F_LINEARIZE_AT)
    ctx.solve_fixed(grid)
    ctx.smooth()
    assert ctx.get(host.F_LINEARIZE_AT).shape == (17, 3, N)
    with pytest.raises(pkg.OdefError, match="fixed grids"):
        ctx.solve_adaptive(0.1, dt0=1e-3, max_steps=64)
    with pytest.raises(pkg.OdefError, match="another grid"):
        ctx.solve_fixed(np.arange(33) * 2.0**-8)
    ctx.solve_fixed(grid)  # the same grid: the next iteration
    assert "ieks" in ctx.kernel_name(0)
    # an undersized bound buffer; odef_set_problem empties the field
    import torch

    small = torch.zeros(16 * 3 * N, dtype=torch.float64, device="cuda")
    ctx.bind_device(host.F_LINEARIZE_AT, small.data_ptr(), small.numel() * 8)
    with pytest.raises(pkg.OdefError, match="bound ODEF_F_LINEARIZE_AT buffer"):
        ctx.solve_fixed(grid)
    ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-2)
    ctx.solve_fixed(grid)
    assert "ieks" not in ctx.kernel_name(0)
    ctx.close()
    # the field belongs to IEKS contexts
    ek1 = pkg.Context("lorenz63", 3, host.EK1_ID, N, smooth=True)
    with pytest.raises(pkg.OdefError, match="IEKS context"):
        ek1.bind_device(host.F_LINEARIZE_AT, small.data_ptr(), small.numel() * 8)
    ek1.close()


def test_ieks_group_two_shards(pkg):
    """solve_ieks on two shards of one ensemble (on this device) against one context: bit for bit, every shard on the row-team
    kernels as the single context."""
    from odefilters_jl_amd import host

    vf = orc.vector_field("lorenz63")
    N = 1001
    grid = np.arange(65) * 2.0**-8
    with host.DeviceGroup("lorenz63", 3, host.IEKS_ID, N, 2, device_ids=[0, 0], smooth=True) as grp:
        grp.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-2)
        grp.solve_ieks(grid, iterations=4)
        gs = grp.gather_field(host.F_SMOOTH_MEAN)
        gm = grp.gather_field(host.F_MEAN)
        glin = grp.gather_field(host.F_LINEARIZE_AT)
        kn = []
        for g in range(2):
            buf = C.create_string_buffer(256)
            grp.lib.odef_kernel_name(grp.lib.odef_group_ctx(grp._h, g), 0, buf, 256)
            kn.append(buf.value.decode())
    ctx = pkg.Context("lorenz63", 3, host.IEKS_ID, N, smooth=True)
    ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-2)
    for _ in range(4):
        ctx.solve_fixed(grid)
        ctx.smooth()
    assert kn == [ctx.kernel_name(0)] * 2 and "ek_filter_rows_ieks_kernel" in kn[0]
    np.testing.assert_array_equal(gs, ctx.get(host.F_SMOOTH_MEAN))
    np.testing.assert_array_equal(gm, ctx.get(host.F_MEAN))
    np.testing.assert_array_equal(glin, ctx.get(host.F_LINEARIZE_AT))
    ctx.close()
