"""Data log-likelihood at arbitrary observation times on the device (ODEF_L_OBS_TIME) against the
extended-precision reference of the augmented chain (tests/_datalik_times_reference.py) applied to the records the same context
returns (MEAN, COV_TRIL, DIFFUSION, T, NSAVED).  Tolerance: 16 C_NUMPY in units of `unit_bound`.  Every test prints its worst
error / unit bound ratios before it returns."""
import numpy as np
import pytest

import _datalik_reference as dr
import _datalik_times_reference as tr
from _datalik_reference import orc

pytestmark = pytest.mark.gpu


def _host():
    from odefilters_jl_amd import host

    return host


def _u0s(N, base, seed, scale=1e-2):
    base = np.asarray(base, float)
    return base[None, :] * (1.0 + scale * np.random.default_rng(seed).standard_normal((N, len(base))))


def _records(ctx, adaptive):
    h = _host()
    ns = ctx.get(h.F_NSAVED) if adaptive else None
    return ctx.get(h.F_MEAN), ctx.get(h.F_COV_TRIL), ctx.get(h.F_DIFFUSION), ctx.get(h.F_T), ns


def _bind(ctx, times, comps, y, r):
    """Uploads the observations (y [M, o] or [N, M, o]) and binds them by time; returns the tensors, which the caller keeps alive."""
    h = _host()
    y = np.asarray(y, float)
    per = y.ndim == 3
    vals = y.transpose(1, 2, 0) if per else y
    bufs = h._to_device((np.asarray(times, np.float64), np.asarray(comps, np.int64), vals, np.asarray(r, float)), ctx.cfg.device)
    ctx.bind_observation_times(*[b.data_ptr() for b in bufs], len(times), len(comps), per)
    return bufs


def _check(ctx, adaptive, times, comps, r, per_traj, seed, label):
    mean, cov, diff, t, ns = _records(ctx, adaptive)
    times = np.asarray(times(t[: ns[0], 0] if adaptive else t), float)
    r = np.broadcast_to(np.asarray(r, float), (len(comps),)).copy()
    y = tr.observations(mean, t, ns, times, comps, r, per_traj, seed)
    keep = _bind(ctx, times, comps, y, r)
    ll, mq = ctx.data_loglik()
    assert ll.shape == mq.shape == (ctx.N,)
    args = (mean, cov, diff, t, ctx.d, ctx.q, times, list(comps), y, r, ns)
    ref, bound = tr.evaluate(*args), tr.unit_bound(*args)
    # the calibration on these very records: the numpy float64 evaluation meets C_NUMPY, so the input is one the constant speaks for
    f64 = dr.ratios(tr.evaluate(*args, dtype=np.float64), ref, bound)
    print(f"{label}: numpy float64 / unit bound", {k: f"{v:.3g}" for k, v in f64.items()}, f"(C_NUMPY = {tr.C_NUMPY})")
    assert max(f64.values()) <= tr.C_NUMPY, (label, "ill-conditioned input: the numpy float64 evaluation misses C_NUMPY", f64)
    rt = tr.check({"loglik": ll, "mahalanobis": mq}, ref, bound, label=label)
    rel = np.max(np.abs(ll - ref["loglik"].astype(float)) / np.abs(ref["loglik"].astype(float)))
    print(f"{label}: error / unit bound", {k: f"{v:.3g}" for k, v in rt.items()},
          f"allowed {tr.DEVICE_FACTOR * tr.C_NUMPY:.3g}; worst relative error of loglik {rel:.3g}; saves "
          f"{(ns.min(), ns.max()) if adaptive else len(t)}")
    assert np.all(np.isfinite(ll)) and np.all(mq >= 0)
    assert ctx.kernel_name(4) == f"odef::data_loglik_times_kernel<{ctx.d}, {ctx.q}>" and ctx.kernel_time_ms(4)[0] > 0
    del keep
    return ll, mq


def _run(pkg, name, N, seed, field=None, u0=None, p=None, max_steps=512):
    """Problem `name` of `_datalik_times_reference.GPU_PROBLEMS` on N trajectories."""
    h = _host()
    fld, kind, order, diffusion, t1, adaptive, dt, times, comps, r, per_traj = tr.GPU_PROBLEMS[name]
    vf = orc.vector_field(fld)
    with pkg.Context(field or fld, order, h.EK1_ID if kind == "EK1" else h.EK0_ID, N, diffusion=diffusion) as ctx:
        ctx.set_problem(_u0s(N, vf.u0 if u0 is None else u0, seed), vf.p if p is None else p, 0.0)
        if adaptive:
            ctx.solve_adaptive(t1, dt0=dt, max_steps=max_steps)
            assert np.all(ctx.get(h.F_RETCODE) == 0)
        else:
            ctx.solve_fixed(np.arange(int(round(t1 / dt)) + 1) * dt)
        out = _check(ctx, adaptive, times, comps, r, per_traj, seed + 100, f"{name} N={N}")
        return out, ctx.kernel_name(0)


def test_lotka_volterra_fixed_grid_times_off_the_grid(pkg):
    """dt = 2^-4 on [0, 2]; seven times: two in one step, one on a save, one a nextafter below a save; components (0, 1)."""
    _run(pkg, "lv-ek1q3-fixed", 130, 1)


def test_lotka_volterra_adaptive_per_trajectory_values(pkg):
    (ll, _), _ = _run(pkg, "lv-ek1q3-adaptive", 66, 2)
    assert len(set(ll)) == 66


@pytest.mark.parametrize("name", ["lorenz-ek1q3-adaptive", "lorenz-ek1q3-map-adaptive"])
def test_lorenz_adaptive_components_0_and_2(pkg, name):
    _run(pkg, name, 65, 3, u0=orc.vector_field("lorenz63").u0 + np.array([0.0, 1.0, 1.0]))


def test_lorenz_adaptive_times_shortly_above_saves(pkg):
    """About one time per step, each 1e-6 to 1e-3 of the step above a save of trajectory 0 and none the first of the set: every
    trajectory gets a finite number within the bound (a node is carried to the save below it without factoring its prediction)."""
    (ll, mq), _ = _run(pkg, "lorenz-ek1q3-adaptive-above-saves", 65, 6, u0=orc.vector_field("lorenz63").u0 + np.array([0.0, 1.0, 1.0]))
    assert np.all(np.isfinite(ll)) and np.all(np.isfinite(mq))


def test_fhn_ek0_q5_adaptive(pkg):
    """D = 12: the largest state the pass serves."""
    _run(pkg, "fhn-ek0q5-adaptive", 65, 4)


def test_records_of_the_row_team_filter(pkg):
    _, filt = _run(pkg, "linear-ek0q1-fixed", 1, 5)
    assert "ek_filter_rows_kernel" in filt


USER4 = """
struct DataLikT4 {
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


def test_run_time_compiled_field_d4_q2_adaptive(pkg):
    """The kernels depend on (d, q) only: a run-time compiled field is served by the instance compiled into the library."""
    h = _host()
    pkg.compile_rhs("DataLikT4", USER4, 4, 2)
    N = 70
    with pkg.Context("DataLikT4", 2, h.EK1_ID, N) as ctx:
        ctx.set_problem(_u0s(N, [1.0, -0.5, 0.0, 0.3], 7), np.array([2.0, 0.5]), 0.0)
        ctx.solve_adaptive(0.75, dt0=2.0 ** -5, max_steps=512)
        assert np.all(ctx.get(h.F_RETCODE) == 0)
        _check(ctx, True, lambda t: tr._late(0.4, 0.75, 4), (1, 3), 1e-3, True, 34, "run-time compiled d=4 EK1(2) adaptive N=70")


def test_times_on_the_grid_through_both_paths(pkg):
    """The same on-grid observations through the time path and through the save path: both within the bound of the save path's
    reference (on the grid the augmented chain is the records)."""
    h = _host()
    vf = orc.vector_field("lorenz63")
    N = 70
    with pkg.Context("lorenz63", 3, h.EK1_ID, N) as ctx:
        ctx.set_problem(_u0s(N, vf.u0 + np.array([0.0, 1.0, 1.0]), 8), vf.p, 0.0)
        ctx.solve_fixed(np.arange(17) * 2.0 ** -6)
        mean, cov, diff, t, _ = _records(ctx, False)
        saves, comps, r = [0, 3, 8, 16], [0, 2], np.full(2, 1e-2)
        y = dr._observations(mean, saves, comps, r, False, 41)
        args = (mean, cov, diff, t, 3, 3, saves, comps, y, r)
        ref, bound = dr.evaluate(*args), dr.unit_bound(*args)
        keep = _bind(ctx, t[saves], comps, y, r)
        a = ctx.data_loglik()
        assert "data_loglik_times_kernel" in ctx.kernel_name(4)
        bufs = h._to_device((np.asarray(saves, np.int64), np.asarray(comps, np.int64), y, r), ctx.cfg.device)
        ctx.bind_observations(*[b.data_ptr() for b in bufs], len(saves), len(comps), False)   # (unbinds the times)
        b = ctx.data_loglik()
        assert ctx.kernel_name(4) == "odef::data_loglik_kernel<3, 3>"
        for label, got in (("time path", a), ("save path", b)):
            rt = dr.check({"loglik": got[0], "mahalanobis": got[1]}, ref, bound, label=label)
            print(f"on-grid times, {label}: error / unit bound", {k: f"{v:.3g}" for k, v in rt.items()})
        del keep, bufs


def test_a_trajectory_that_ends_before_the_last_time_gives_nan(pkg):
    """Lotka-Volterra EK1(3), adaptive, 60 steps at most.  By the oracle's solves of the same inputs the trajectories with the
    parameters p take 40 attempts to reach t = 2 and those with 2 p take 84 (they are near t = 1.4 after 60): NaN exactly for the
    latter."""
    h = _host()
    vf = orc.vector_field("lotka_volterra")
    N = 6
    fast = np.arange(N) % 2 == 1
    ps = np.where(fast[:, None], 2.0, 1.0) * np.asarray(vf.p)[None, :]
    with pkg.Context("lotka_volterra", 3, h.EK1_ID, N, params_shared=False) as ctx:
        ctx.set_problem(_u0s(N, vf.u0, 9, 1e-3), ps, 0.0)
        ctx.solve_adaptive(2.0, dt0=2.0 ** -6, max_steps=60)
        mean, cov, diff, t, ns = _records(ctx, True)
        t_end = t[ns - 1, np.arange(N)]
        times = np.array([0.9, 1.31, 1.9])
        assert np.all(t_end[fast] < times[-1]) and np.all(t_end[~fast] >= times[-1]), (t_end, ns)
        assert np.all(ctx.get(h.F_RETCODE)[fast] != 0) and np.all(ctx.get(h.F_RETCODE)[~fast] == 0)
        r = np.full(2, 1e-2)
        y = tr.observations(mean, t, ns, times, (0, 1), r, False, 42)
        keep = _bind(ctx, times, (0, 1), y, r)
        ll, mq = ctx.data_loglik()
        assert np.array_equal(np.isnan(ll), fast) and np.array_equal(np.isnan(mq), fast)
        args = (mean, cov, diff, t, 2, 3, times, [0, 1], y, r, ns)
        tr.check({"loglik": ll, "mahalanobis": mq}, tr.evaluate(*args), tr.unit_bound(*args), label="ends early")
        del keep


def test_cache_and_rebinding_the_times(pkg):
    h = _host()
    vf = orc.vector_field("lorenz63")
    N = 70
    with pkg.Context("lorenz63", 2, h.EK1_ID, N) as ctx:
        ctx.set_problem(_u0s(N, vf.u0, 8), vf.p, 0.0)
        ctx.solve_adaptive(0.125, dt0=2.0 ** -7, max_steps=256)
        mean, cov, diff, t, ns = _records(ctx, True)
        times, comps, r = np.array([0.04, 0.1]), [0, 1, 2], np.full(3, 1e-2)
        y = tr.observations(mean, t, ns, times, comps, r, False, 40)
        keep = _bind(ctx, times, comps, y, r)
        n0 = ctx.kernel_time_ms(4)[1]
        a = ctx.data_loglik()
        b = ctx.data_loglik()
        assert ctx.kernel_time_ms(4)[1] == n0 + 1                              # the second request launched nothing
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        ptr, nbytes = ctx.device_ptr(h.L_DATA_LOGLIK)
        assert nbytes == 8 * N and ctx.kernel_time_ms(4)[1] == n0 + 1
        other = h._to_device((times + 0.003,), ctx.cfg.device)[0]             # rebinding TIME recomputes
        ctx.bind_device(h.L_OBS_TIME, other.data_ptr(), other.numel() * 8)
        c = ctx.data_loglik()
        assert ctx.kernel_time_ms(4)[1] == n0 + 2 and not np.array_equal(c[0], a[0])
        args = (mean, cov, diff, t, 3, 2, times + 0.003, comps, y, r, ns)
        tr.check({"loglik": c[0], "mahalanobis": c[1]}, tr.evaluate(*args), tr.unit_bound(*args), label="rebound")
        del keep


def test_refusals(pkg):
    h = _host()
    vf = orc.vector_field("lorenz63")
    N, grid = 3, np.arange(5) * 2.0 ** -6
    dev = lambda *a: h._to_device(a, -1)  # noqa: E731
    tm, cp, vl, ns = dev(np.array([0.01, 0.05]), np.array([0, 2], np.int64), np.zeros((2, 2)), np.array([1e-2, 1e-2]))
    sv = dev(np.array([1, 4], np.int64))[0]
    fields = (h.L_OBS_TIME, h.L_OBS_COMPONENT, h.L_OBS_VALUE, h.L_OBS_NOISE)

    def bind(ctx, t=tm, c=cp, v=vl, n=ns):
        for f, b in zip(fields, (t, c, v, n)):
            ctx.bind_device(f, b.data_ptr() if b is not None else 0, b.numel() * 8 if b is not None else 0)

    with pkg.Context("lorenz63", 2, h.EK1_ID, N) as ctx:
        ctx.set_problem(_u0s(N, vf.u0, 9), vf.p, 0.0)
        bind(ctx)
        with pytest.raises(pkg.OdefError, match="before a solve"):
            ctx.data_loglik()
        ctx.solve_adaptive(float(grid[-1]), dt0=2.0 ** -6, max_steps=64)
        assert np.all(np.isfinite(ctx.data_loglik()[0]))                      # allowed after an adaptive solve ...
        ctx.solve_fixed(grid)
        assert np.all(np.isfinite(ctx.data_loglik()[0]))                      # ... and after a fixed one
        ctx.bind_device(h.L_OBS_SAVE, sv.data_ptr(), 16)
        with pytest.raises(pkg.OdefError, match="ODEF_L_OBS_SAVE and ODEF_L_OBS_TIME are both bound"):
            ctx.data_loglik()
        ctx.bind_device(h.L_OBS_SAVE, 0, 0)                                    # NULL unbinds
        assert np.all(np.isfinite(ctx.data_loglik()[0]))
        bind(ctx, v=None)
        with pytest.raises(pkg.OdefError, match="input missing.*ODEF_L_OBS_VALUE"):
            ctx.data_loglik()
        bind(ctx, v=dev(np.zeros(5))[0])
        with pytest.raises(pkg.OdefError, match="byte counts do not agree"):
            ctx.data_loglik()
        for t, msg in ((np.array([0.01, np.inf]), "must be finite"), (np.array([np.nan, 0.02]), "must be finite"),
                       (np.array([0.03, 0.03]), "strictly increasing"), (np.array([0.05, 0.01]), "strictly increasing"),
                       (np.array([-1e-3, 0.01]), "before the first save"),
                       (np.array([0.01, np.nextafter(grid[-1], 1.0)]), "above the last save of the grid")):
            bind(ctx, t=dev(t)[0])
            with pytest.raises(pkg.OdefError, match=msg):
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
    with pkg.Context("lorenz63", 5, h.EK1_ID, N) as ctx:                       # D = 18: the save path has a kernel, this one not
        ctx.set_problem(_u0s(N, vf.u0, 9), vf.p, 0.0)
        ctx.solve_fixed(grid)
        bind(ctx)
        with pytest.raises(pkg.OdefError, match=r"no kernel for \(d, q\) = \(3, 5\).*d \(q \+ 1\) <= 12"):
            ctx.data_loglik()
    l96 = orc.vector_field("lorenz96")
    with pkg.Context("lorenz96", 1, h.EK0_ID, 2) as ctx:                       # the workgroup-per-trajectory path
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
    times = np.array([0.0, 0.3, 0.31, 0.74])
    shared = rng.standard_normal((4, 1))
    per = rng.standard_normal((N, 4, 1))
    with h.DeviceGroup("fhn", 2, h.EK1_ID, N, 2, device_ids=[0, 0]) as grp, pkg.Context("fhn", 2, h.EK1_ID, N) as ctx:
        for adaptive in (False, True):
            for c in (grp, ctx):
                c.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-2)
                if adaptive:
                    c.solve_adaptive(0.75, dt0=2.0 ** -5, max_steps=256)
                else:
                    c.solve_fixed(grid)
            sol = pkg.EnsembleSolution(ctx, pkg.EK1(order=2, smooth=False), adaptive)
            for data in (shared, per):
                g = grp.data_loglik(times, data, 0.5, components=(1,))
                s = sol.data_loglik(times, data, 0.5, components=(1,))
                assert "data_loglik_times_kernel" in ctx.kernel_name(4)
                assert g[0].shape == (N,) and np.all(np.isfinite(g[0]))
                assert g[0].tobytes() == s[0].tobytes() and g[1].tobytes() == s[1].tobytes()


def test_inference_on_an_adaptive_ensemble(pkg):
    """Lotka-Volterra EK1(3), adaptive, 33 candidates of p[0] around 1.5; data: a tight oracle solve at 1.5 plus seeded noise at 16
    times that are no save of any candidate.  The best candidate lies within one index of the truth."""
    from test_datalik_times_reference import inference_inputs

    vf, ps, times, data, sigma = inference_inputs()
    N = len(ps)
    prob = pkg.EnsembleProblem(pkg.ODEProblem("lotka_volterra", vf.u0, (0.0, 2.0), vf.p), u0s=np.tile(vf.u0, (N, 1)), ps=ps)
    sol = pkg.solve(prob, pkg.EK1(order=3, smooth=False), pkg.EnsembleHIP(), adaptive=True, dt=2.0 ** -6, max_steps=512)
    ll, mq = sol.data_loglik(times, data, sigma ** 2)
    best = int(np.argmax(ll))
    print(f"argmax {best} of {N} (truth at {(N - 1) // 2}); mahalanobis {mq[best]:.2f} for {data.size} degrees of freedom; "
          f"loglik {ll[best]:.4g}, at the ends {ll[0]:.3g} {ll[-1]:.3g}")
    assert np.all(np.isfinite(ll)) and abs(best - (N - 1) // 2) <= 1


def test_through_solve_adaptive_and_off_grid_times_return_numbers(pkg):
    """Both raised before the time path existed."""
    vf = orc.vector_field("lotka_volterra")
    N = 5
    prob = pkg.EnsembleProblem(pkg.ODEProblem("lotka_volterra", vf.u0, (0.0, 1.0), vf.p), perturb_scale=1e-2)
    data = np.tile(vf.u0, (2, 1))
    sol = pkg.solve(prob, pkg.EK1(order=3, smooth=False), pkg.EnsembleHIP(), trajectories=N, adaptive=True)
    ll, mq = sol.data_loglik([0.013, 0.4], data, 0.25)
    assert ll.shape == (N,) and np.all(np.isfinite(ll)) and np.all(mq >= 0)
    sol = pkg.solve(prob, pkg.EK1(order=3, smooth=False), pkg.EnsembleHIP(), trajectories=N, adaptive=False, dt=2.0 ** -4)
    ll, mq = sol.data_loglik([0.013, 0.4], data, 0.25)
    assert np.all(np.isfinite(ll)) and "data_loglik_times_kernel" in sol.ctx.kernel_name(4)
    on = sol.data_loglik([0.25, 0.5], data, 0.25)                             # on the grid: the save path, as before
    assert np.all(np.isfinite(on[0])) and sol.ctx.kernel_name(4) == "odef::data_loglik_kernel<2, 3>"
    with pytest.raises(pkg.OdefError, match="above the last save"):
        sol.data_loglik([0.4, 1.0 + 1e-9], data, 0.25)
