"""Data log-likelihood of noisy observations on the device (odef_data_field) against the extended-precision
reference of tests/_datalik_reference.py applied to the records the same context returns (MEAN, COV_TRIL, DIFFUSION, T).
Tolerance: 16 times the measured error of the numpy float64 evaluation (`_datalik_reference.C_NUMPY`), in units of
`unit_bound`.  Every test prints its worst error / unit bound ratios before it returns."""
import numpy as np
import pytest

import _datalik_reference as dr
from _datalik_reference import orc

pytestmark = pytest.mark.gpu


def _host():
    from odefilters_jl_amd import host

    return host


def _u0s(N, base, seed, scale=1e-2):
    base = np.asarray(base, float)
    return base[None, :] * (1.0 + scale * np.random.default_rng(seed).standard_normal((N, len(base))))


def _records(ctx):
    h = _host()
    return ctx.get(h.F_MEAN), ctx.get(h.F_COV_TRIL), ctx.get(h.F_DIFFUSION), ctx.get(h.F_T)


def _bind(ctx, saves, comps, y, r):
    """Uploads the observations (y [M, o] or [N, M, o]) and binds them; returns the tensors, which the caller keeps alive."""
    h = _host()
    y = np.asarray(y, float)
    per = y.ndim == 3
    vals = y.transpose(1, 2, 0) if per else y
    bufs = h._to_device((np.asarray(saves, np.int64), np.asarray(comps, np.int64), vals, np.asarray(r, float)), ctx.cfg.device)
    ctx.bind_observations(*[b.data_ptr() for b in bufs], len(saves), len(comps), per)
    return bufs


def _check(ctx, saves, comps, r, per_traj, seed, label):
    mean, cov, diff, t = _records(ctx)
    saves = [s if s >= 0 else len(t) + s for s in saves]
    r = np.broadcast_to(np.asarray(r, float), (len(comps),)).copy()
    y = dr._observations(mean, saves, comps, r, per_traj, seed)
    keep = _bind(ctx, saves, comps, y, r)
    ll, mq = ctx.data_loglik()
    assert ll.shape == mq.shape == (ctx.N,)
    args = (mean, cov, diff, t, ctx.d, ctx.q, saves, list(comps), y, r)
    ref = dr.evaluate(*args)
    rt = dr.check({"loglik": ll, "mahalanobis": mq}, ref, dr.unit_bound(*args), label=label)
    f64 = dr.ratios(dr.evaluate(*args, dtype=np.float64), ref, dr.unit_bound(*args))
    rel = np.max(np.abs(ll - ref["loglik"].astype(float)) / np.abs(ref["loglik"].astype(float)))
    print(f"{label}: error / unit bound", {k: f"{v:.3g}" for k, v in rt.items()}, "numpy float64:", {k: f"{v:.3g}" for k, v in f64.items()},
          f"allowed {dr.DEVICE_FACTOR * dr.C_NUMPY:.3g}; worst relative error of loglik {rel:.3g}")
    assert np.all(np.isfinite(ll)) and np.all(mq >= 0)
    assert ctx.kernel_name(4) == f"odef::data_loglik_kernel<{ctx.d}, {ctx.q}>" and ctx.kernel_time_ms(4)[0] > 0
    del keep
    return ll, mq


@pytest.mark.parametrize("q", [1, 2, 3, 4])
def test_linear_ek0(pkg, q):
    h = _host()
    vf = orc.vector_field("linear")
    N = 130
    with pkg.Context("linear", q, h.EK0_ID, N) as ctx:
        ctx.set_problem(_u0s(N, vf.u0, q), vf.p, 0.0)
        ctx.solve_fixed(np.arange(10) * 0.125)
        _check(ctx, range(10), (0, 1), 1e-4, False, 20 + q, f"linear EK0({q}) N=130")


def test_fhn_ek1_q3(pkg):
    h = _host()
    vf = orc.vector_field("fhn")
    N = 65
    with pkg.Context("fhn", 3, h.EK1_ID, N) as ctx:
        ctx.set_problem(_u0s(N, vf.u0, 3), vf.p, 0.0)
        ctx.solve_fixed(np.arange(17) * 0.0625)
        _check(ctx, range(0, 17, 4), (1,), 1e-3, False, 30, "fhn EK1(3) N=65")


def test_lorenz_ek1_q3_components_0_and_2(pkg):
    h = _host()
    vf = orc.vector_field("lorenz63")
    N = 130
    with pkg.Context("lorenz63", 3, h.EK1_ID, N) as ctx:
        ctx.set_problem(_u0s(N, vf.u0 + np.array([0.0, 1.0, 1.0]), 4), vf.p, 0.0)
        ctx.solve_fixed(np.arange(33) * 2.0 ** -6)
        _check(ctx, range(0, 33, 4), (0, 2), 1e-2, False, 31, "lorenz EK1(3) N=130 33 saves c=(0,2)")
        assert "ek_filter_rows" in ctx.kernel_name(0)


@pytest.mark.parametrize("diffusion", ["dynamic", "fixedMAP"])
def test_lorenz_ek1_q5(pkg, diffusion):
    """D = 18: records of the lane filter (the row teams stop at D = 16); the kernel above the lane smoother's D = 12."""
    h = _host()
    vf = orc.vector_field("lorenz63")
    N = 64
    with pkg.Context("lorenz63", 5, h.EK1_ID, N, diffusion=diffusion) as ctx:
        ctx.set_problem(_u0s(N, vf.u0 + np.array([0.0, 1.0, 1.0]), 5), vf.p, 0.0)
        ctx.solve_fixed(np.arange(17) * 2.0 ** -5)
        _check(ctx, (4, 9, -1), (0, 1, 2), 1e-2, False, 32, f"lorenz EK1(5) {diffusion} N=64 17 saves")
        assert "rows" not in ctx.kernel_name(0)


def test_per_trajectory_values(pkg):
    h = _host()
    vf = orc.vector_field("fhn")
    N = 130
    with pkg.Context("fhn", 1, h.EK1_ID, N, diffusion="fixed") as ctx:
        ctx.set_problem(_u0s(N, vf.u0, 6), vf.p, 0.0)
        ctx.solve_fixed(np.arange(17) * 0.0625)
        ll, _ = _check(ctx, range(0, 17, 4), (0, 1), (1e-3, 4e-3), True, 33, "fhn EK1(1) fixed N=130 per-trajectory values")
        assert len(set(ll)) == N


USER4 = """
struct DataLik4 {
  static constexpr int d = 4, np = 2;
  template <class T>
  __device__ static void f(const T (&u)[4], const double* p, T (&du)[4]) {
    du[0] = u[2];
    du[1] = u[3];
    du[2] = -p[0] * u[0] + p[1] * (u[1] - u[0]);
    du[3] = -p[0] * u[1] + p[1] * (u[0] - u[1]) * u[0];
  }
};
"""


def test_run_time_compiled_field_d4_q2(pkg):
    """The kernels depend on (d, q) only: a run-time compiled field is served by the instance compiled into the library."""
    h = _host()
    pkg.compile_rhs("DataLik4", USER4, 4, 2)
    N = 70
    with pkg.Context("DataLik4", 2, h.EK1_ID, N) as ctx:
        ctx.set_problem(_u0s(N, [1.0, -0.5, 0.0, 0.3], 7), np.array([2.0, 0.5]), 0.0)
        ctx.solve_fixed(np.arange(13) * 0.0625)
        assert np.all(ctx.get(h.F_RETCODE) == 0)
        _check(ctx, (0, 6, 12), (1, 3), 1e-3, True, 34, "run-time compiled d=4 EK1(2) N=70")


def test_records_of_the_row_team_filter(pkg):
    """dispatch: the row-team filter serves every ensemble below 12 288 trajectories at D <= 16 (rows_launch.h), so the smallest
    such context has one trajectory."""
    h = _host()
    vf = orc.vector_field("lotka_volterra")
    with pkg.Context("lotka_volterra", 3, h.EK0_ID, 1) as ctx:
        ctx.set_problem(np.asarray(vf.u0)[None, :], vf.p, 0.0)
        ctx.solve_fixed(np.arange(12) * 0.0625)
        assert "ek_filter_rows_kernel" in ctx.kernel_name(0)
        _check(ctx, (5,), (1,), 1e-2, False, 35, "lotka-volterra EK0(3) N=1, row-team filter")


def test_inference_picks_the_parameter_that_generated_the_data(pkg):
    """Lotka-Volterra EK1(3), 256 candidates of p[0] swept linearly around 1.5; data: a tight oracle solve at 1.5 plus seeded
    N(0, 1e-4) noise.  The best candidate lies within two grid cells of the truth and is calibrated."""
    vf = orc.vector_field("lotka_volterra")
    N, sigma = 256, 1e-2
    grid = np.arange(65) * 2.0 ** -5
    obs = np.arange(4, 65, 4)
    tight = orc.solve(vf, orc.EK1(order=4, smooth=False), tgrid=np.arange(2 * 256 + 1) * 2.0 ** -8)
    truth = tight.means(False)[:: 8][obs][:, :2]                                   # u at the observation times
    assert np.array_equal(np.asarray(tight.t)[:: 8][obs], grid[obs])
    data = truth + sigma * np.random.default_rng(2022).standard_normal(truth.shape)
    ps = np.tile(vf.p, (N, 1))
    ps[:, 0] = np.linspace(1.2, 1.8, N)
    prob = pkg.EnsembleProblem(pkg.ODEProblem("lotka_volterra", vf.u0, (0.0, 2.0), vf.p), u0s=np.tile(vf.u0, (N, 1)), ps=ps)
    sol = pkg.solve(prob, pkg.EK1(order=3, smooth=False), pkg.EnsembleHIP(), tstops=grid, adaptive=False)
    ll, mq = sol.data_loglik(grid[obs], data, sigma ** 2)
    best = int(np.argmax(ll))
    true_index = (1.5 - 1.2) / (0.6 / (N - 1))
    dof = data.size
    print(f"argmax {best} (truth at {true_index:.1f}), p = {ps[best, 0]:.5f}; mahalanobis {mq[best]:.2f} for {dof} degrees of freedom; "
          f"loglik {ll[best]:.3f}, at the ends {ll[0]:.1f} {ll[-1]:.1f}")
    assert abs(best - true_index) <= 2
    assert abs(mq[best] - dof) <= 5 * np.sqrt(2 * dof)
    with pytest.raises(pkg.OdefError, match="exactly"):
        sol.data_loglik(grid[obs] + 1e-9, data, sigma ** 2)


def test_cache_and_invalidation(pkg):
    import torch

    h = _host()
    vf = orc.vector_field("lorenz63")
    N = 70
    with pkg.Context("lorenz63", 2, h.EK1_ID, N) as ctx:
        ctx.set_problem(_u0s(N, vf.u0, 8), vf.p, 0.0)
        ctx.solve_fixed(np.arange(9) * 2.0 ** -6)
        mean = ctx.get(h.F_MEAN)
        saves, comps, r = [2, 8], [0, 1, 2], np.full(3, 1e-2)
        y = dr._observations(mean, saves, comps, r, False, 40)
        keep = _bind(ctx, saves, comps, y, r)
        a = ctx.data_loglik()
        n1 = ctx.kernel_time_ms(4)[1]
        b = ctx.data_loglik()
        assert n1 == 1 and ctx.kernel_time_ms(4)[1] == 1                      # the second request launched nothing
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        ptr, nbytes = ctx.device_ptr(h.L_DATA_LOGLIK)                         # the device copy is the cached array
        assert nbytes == 8 * N and ctx.kernel_time_ms(4)[1] == 1
        vals = h._to_device((y + 0.05,), ctx.cfg.device)[0]                   # rebinding VALUE recomputes
        ctx.bind_device(h.L_OBS_VALUE, vals.data_ptr(), vals.numel() * 8)
        c = ctx.data_loglik()
        assert ctx.kernel_time_ms(4)[1] == 2 and not np.array_equal(c[0], a[0])
        ptr, nbytes = ctx.device_ptr(h.F_COV_TRIL)                            # a writable pointer: the cache goes ...

        class Raw:
            __cuda_array_interface__ = {"shape": (nbytes // 8,), "typestr": "<f8", "data": (ptr, False), "version": 2}

        torch.as_tensor(Raw(), device="cuda").mul_(4.0)                       # ... and the records change under it
        torch.cuda.synchronize()
        d = ctx.data_loglik()
        assert ctx.kernel_time_ms(4)[1] == 3 and not np.array_equal(d[0], c[0])
        mean, cov, diff, t = _records(ctx)
        ref = dr.evaluate(mean, cov, diff, t, 3, 2, saves, comps, y + 0.05, r)
        dr.check({"loglik": d[0], "mahalanobis": d[1]}, ref, dr.unit_bound(mean, cov, diff, t, 3, 2, saves, comps, y + 0.05, r), label="scaled")
        ctx.solve_fixed(np.arange(9) * 2.0 ** -6)                             # a new solve: the records are the unscaled ones again
        e = ctx.data_loglik()
        assert ctx.kernel_time_ms(4)[1] == 4 and e[0].tobytes() == c[0].tobytes()
        del keep


def test_refusals(pkg):
    h = _host()
    vf = orc.vector_field("lorenz63")
    N, grid = 3, np.arange(5) * 2.0 ** -6
    dev = lambda *a: h._to_device(a, -1)  # noqa: E731
    sv, cp, vl, ns = dev(np.array([1, 4], np.int64), np.array([0, 2], np.int64), np.zeros((2, 2)), np.array([1e-2, 1e-2]))

    def bind(ctx, s=sv, c=cp, v=vl, n=ns):
        for f, b in zip((h.L_OBS_SAVE, h.L_OBS_COMPONENT, h.L_OBS_VALUE, h.L_OBS_NOISE), (s, c, v, n)):
            ctx.bind_device(f, b.data_ptr() if b is not None else 0, b.numel() * 8 if b is not None else 0)

    with pkg.Context("lorenz63", 2, h.EK1_ID, N) as ctx:
        ctx.set_problem(_u0s(N, vf.u0, 9), vf.p, 0.0)
        bind(ctx)
        with pytest.raises(pkg.OdefError, match="before a solve"):
            ctx.data_loglik()
        ctx.solve_adaptive(float(grid[-1]), dt0=2.0 ** -6, max_steps=64)
        with pytest.raises(pkg.OdefError, match="observation times are per ensemble.*grid.*per trajectory"):
            ctx.data_loglik()
        ctx.solve_fixed(grid)
        assert np.all(np.isfinite(ctx.data_loglik()[0]))
        bind(ctx, v=None)
        with pytest.raises(pkg.OdefError, match="input missing.*ODEF_L_OBS_VALUE"):
            ctx.data_loglik()
        bind(ctx, v=dev(np.zeros(5))[0])
        with pytest.raises(pkg.OdefError, match="byte counts do not agree"):
            ctx.data_loglik()
        for s in (np.array([4, 1], np.int64), np.array([1, 5], np.int64), np.array([-1, 2], np.int64)):
            bind(ctx, s=dev(s)[0])
            with pytest.raises(pkg.OdefError, match="saves must be strictly increasing within 0 .. n_save - 1 = 4"):
                ctx.data_loglik()
        for c in (np.array([2, 0], np.int64), np.array([0, 3], np.int64)):
            bind(ctx, c=dev(c)[0])
            with pytest.raises(pkg.OdefError, match="components must be strictly increasing within 0 .. d - 1 = 2"):
                ctx.data_loglik()
        for n in (np.array([1e-2, 0.0]), np.array([np.inf, 1.0]), np.array([1.0, np.nan])):
            bind(ctx, n=dev(n)[0])
            with pytest.raises(pkg.OdefError, match="finite and positive"):
                ctx.data_loglik()
        bind(ctx)
        assert np.all(np.isfinite(ctx.data_loglik()[0]))                      # a refusal leaves the context usable
    with pkg.Context("lorenz63", 2, h.EK0_ID, N, diffusion="fixedMV") as ctx:
        ctx.set_problem(_u0s(N, vf.u0, 9), vf.p, 0.0)
        ctx.solve_fixed(grid)
        bind(ctx)
        with pytest.raises(pkg.OdefError, match="dynamicMV / :fixedMV"):
            ctx.data_loglik()
    with pkg.Context("lorenz63", 2, h.EK1_ID, N, save_everystep=False) as ctx:
        ctx.set_problem(_u0s(N, vf.u0, 9), vf.p, 0.0)
        ctx.solve_fixed(grid)
        bind(ctx)
        with pytest.raises(pkg.OdefError, match="kept only the final state"):
            ctx.data_loglik()
    l96 = orc.vector_field("lorenz96")
    with pkg.Context("lorenz96", 1, h.EK0_ID, 2) as ctx:
        ctx.set_problem(_u0s(2, l96.u0, 9, 1e-3), l96.p, 0.0)
        ctx.solve_fixed(np.arange(3) * 2.0 ** -7)
        bind(ctx)
        with pytest.raises(pkg.OdefError, match=r"no kernel for \(d, q\) = \(16, 1\)"):
            ctx.data_loglik()


def test_group_on_one_device_equals_the_context(pkg):
    h = _host()
    vf = orc.vector_field("fhn")
    N, grid = 131, np.arange(13) * 0.0625
    rng = np.random.default_rng(41)
    times = grid[[0, 5, 12]]
    shared = rng.standard_normal((3, 1))
    per = rng.standard_normal((N, 3, 1))
    with h.DeviceGroup("fhn", 2, h.EK1_ID, N, 2, device_ids=[0, 0]) as grp, pkg.Context("fhn", 2, h.EK1_ID, N) as ctx:
        for c in (grp, ctx):
            c.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-2)
            c.solve_fixed(grid)
        sol = pkg.EnsembleSolution(ctx, pkg.EK1(order=2, smooth=False), False)
        for data in (shared, per):
            g = grp.data_loglik(times, data, 0.5, components=(1,))
            s = sol.data_loglik(times, data, 0.5, components=(1,))
            assert g[0].shape == (N,) and g[0].tobytes() == s[0].tobytes() and g[1].tobytes() == s[1].tobytes()
    with h.DeviceGroup("fhn", 2, h.EK1_ID, N, 1) as one, pkg.Context("fhn", 2, h.EK1_ID, N) as ctx:
        for c in (one, ctx):
            c.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-2)
            c.solve_fixed(grid)
        g = one.data_loglik(times, per, 0.5, components=(1,))
        s = pkg.EnsembleSolution(ctx, pkg.EK1(order=2, smooth=False), False).data_loglik(times, per, 0.5, components=(1,))
        assert g[0].tobytes() == s[0].tobytes() and g[1].tobytes() == s[1].tobytes()
