"""Event location on the device (odef_event_field) against the definition of tests/_events_reference.py -- bracket
rule, plain bisection to adjacent doubles, oracle.dense_output -- applied to the records the same context returns (MEAN, COV_TRIL,
DIFFUSION, T, NSAVED and the smoothed ones).  Bounds: the module docstring of _events_reference (the dense-output bar carried to
the time axis); every event of every trajectory is checked.  Every test prints its worst ratios and NEVAL statistics."""
import numpy as np
import pytest
from scipy.integrate import solve_ivp

import _events_reference as er

orc = er.orc
pytestmark = pytest.mark.gpu


def _host():
    from odefilters_jl_amd import host

    return host


def _records(ctx, adaptive=False, smoothed=True):
    h = _host()
    n, N = ctx.n_save, ctx.N
    rec = dict(mean=ctx.get(h.F_MEAN).reshape(n, ctx.D, N), cov=ctx.get(h.F_COV_TRIL).reshape(n, ctx.TRI, N),
               diff=ctx.get(h.F_DIFFUSION).reshape(n, N), d=ctx.d, q=ctx.q)
    t = ctx.get(h.F_T)
    rec["t"] = t.reshape(n, N) if adaptive else t.reshape(n)
    rec["nsaved"] = ctx.get(h.F_NSAVED).astype(np.int32) if adaptive else np.full(N, n, np.int32)
    if smoothed:
        rec["smean"] = ctx.get(h.F_SMOOTH_MEAN).reshape(n, ctx.D, N)
        rec["scov"] = ctx.get(h.F_SMOOTH_COV_TRIL).reshape(n, ctx.TRI, N)
    return rec


def _bind(ctx, c, levels, direction, K):
    """Uploads spec and level and binds them; returns the tensors, which the caller keeps alive."""
    h = _host()
    lv = np.atleast_1d(np.asarray(levels, float))
    bufs = h._to_device((np.array([c, direction, K], np.int64), lv), ctx.cfg.device)
    ctx.bind_event(bufs[0].data_ptr(), bufs[1].data_ptr(), lv.size > 1)
    return bufs


def _abi(ctx, source):
    h = _host()
    N, d = ctx.N, ctx.d
    out = {k: ctx.get(h.event_field(source, q)) for q, k in enumerate(er.KEYS)}
    out["u"] = out["u"].reshape(-1, d, N)
    for k in ("time", "tvar", "direction", "save", "neval"):
        out[k] = out[k].reshape(-1, N)
    return out


def _check(ctx, rec, source, c, levels, direction, K, label):
    keep = _bind(ctx, c, levels, direction, K)
    out = _abi(ctx, source)
    assert out["count"].dtype == np.int32 and out["count"].shape == (ctx.N,) and out["time"].shape == (K, ctx.N)
    assert out["u"].shape == (K, ctx.d, ctx.N) and out["save"].dtype == np.int32
    stats = {}
    er.check(rec, out, c, levels, direction, K, bool(source), label=label, stats=stats)
    print(f"{label} source {source} K {K}: counts {out['count'].min()} .. {out['count'].max()};", er.summarize(stats))
    assert ctx.kernel_name(5) == f"odef::event_refine_kernel<{ctx.d}, {ctx.q}>" and ctx.kernel_time_ms(5)[0] > 0
    del keep
    return out


@pytest.fixture(scope="module")
def lv_fixed(pkg):
    """Lotka-Volterra EK1(3), N = 130, dt = 2^-4 on [0, 6], smoothed: solved once, its records fetched once and left unchanged."""
    h = _host()
    vf = orc.vector_field("lotka_volterra")
    ctx = pkg.Context("lotka_volterra", 3, h.EK1_ID, 130)
    ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-2)
    ctx.solve_fixed(np.arange(97) * 2.0 ** -4)
    ctx.smooth()
    yield ctx, _records(ctx)
    ctx.close()


@pytest.mark.parametrize("source", [0, 1])
def test_lotka_volterra_fixed_grid(lv_fixed, source):
    ctx, rec = lv_fixed
    full = _check(ctx, rec, source, 1, 1.0, 0, 6, "lotka-volterra EK1(3) N=130")        # K above the count: NaN slots
    assert full["count"].min() >= 3 and full["count"].max() == 4 and np.all(full["save"][4:] == -1)
    keep = _bind(ctx, 1, 1.0, 0, 2)                                                     # K below the count: truncated
    cut = _abi(ctx, source)
    assert np.array_equal(cut["count"], full["count"]) and cut["time"].shape == (2, 130)
    for k in er.KEYS[1:]:
        assert np.array_equal(cut[k], full[k][:2]), k                                   # the first K in time order, bit for bit
    del keep


def test_directions_and_per_trajectory_levels(lv_fixed):
    ctx, rec = lv_fixed
    lv = 1.0 + 0.02 * np.sin(np.arange(130))
    up = _check(ctx, rec, 1, 1, lv, 1, 3, "lotka-volterra up, per-trajectory levels")
    down = _check(ctx, rec, 1, 1, lv, -1, 3, "lotka-volterra down, per-trajectory levels")
    keep = _bind(ctx, 1, lv, 0, 6)
    both = _abi(ctx, 1)
    assert np.array_equal(up["count"] + down["count"], both["count"])
    assert np.all(up["direction"][up["save"] >= 0] == 1) and np.all(down["direction"][down["save"] >= 0] == -1)
    del keep


def test_lotka_volterra_adaptive(pkg):
    h = _host()
    vf = orc.vector_field("lotka_volterra")
    with pkg.Context("lotka_volterra", 3, h.EK1_ID, 66) as ctx:
        ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-2)
        ctx.solve_adaptive(6.0, abstol=1e-6, reltol=1e-3, dt0=1e-2, max_steps=512)
        ctx.smooth()
        assert np.all(ctx.get(h.F_RETCODE) == 0)
        rec = _records(ctx, adaptive=True)
        assert len(set(rec["nsaved"])) > 1                                              # ragged record counts
        for source in (0, 1):
            out = _check(ctx, rec, source, 1, 1.0, 0, 5, "lotka-volterra adaptive N=66")
            assert out["count"].min() >= 3


def test_lorenz63(pkg):
    h = _host()
    vf = orc.vector_field("lorenz63")
    with pkg.Context("lorenz63", 3, h.EK1_ID, 65) as ctx:
        ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-2)
        ctx.solve_fixed(np.arange(65) * 2.0 ** -6)
        ctx.smooth()
        rec = _records(ctx)
        for source in (0, 1):
            out = _check(ctx, rec, source, 0, 0.0, 0, 2, "lorenz63 EK1(3) N=65")
            assert out["count"].min() >= 1


def test_fhn_ek0_q5_state_dimension_12(pkg):
    h = _host()
    vf = orc.vector_field("fhn")
    with pkg.Context("fhn", 5, h.EK0_ID, 65) as ctx:
        ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-2)
        ctx.solve_fixed(np.arange(49) * 2.0 ** -6)                                  # (EK0(5) on this field is unstable at 2^-4)
        ctx.smooth()
        assert np.all(ctx.get(h.F_RETCODE) == 0)
        rec = _records(ctx)
        for source in (0, 1):
            out = _check(ctx, rec, source, 0, 0.0, 1, 2, "fhn EK0(5) D=12 N=65 up")
            assert out["count"].min() >= 1 and np.all(out["direction"][out["save"] >= 0] == 1)


def test_records_of_the_row_team_filter(pkg):
    h = _host()
    vf = orc.vector_field("linear")
    with pkg.Context("linear", 1, h.EK0_ID, 1) as ctx:
        ctx.set_problem(np.asarray(vf.u0)[None, :], vf.p, 0.0)
        ctx.solve_fixed(np.arange(17) * 2.0 ** -4)
        ctx.smooth()
        assert "ek_filter_rows_kernel" in ctx.kernel_name(0)
        rec = _records(ctx)
        for source in (0, 1):
            out = _check(ctx, rec, source, 0, 0.2, 0, 2, "linear EK0(1) N=1, row-team filter")
            assert out["count"][0] == 1 and out["direction"][0, 0] == 1


USER4 = """
struct Events4 {
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
    pkg.compile_rhs("Events4", USER4, 4, 2)
    N = 70
    base = np.array([1.0, -0.5, 0.0, 0.3])
    u0s = base[None, :] * (1.0 + 1e-2 * np.random.default_rng(7).standard_normal((N, 4)))
    with pkg.Context("Events4", 2, h.EK1_ID, N) as ctx:
        ctx.set_problem(u0s, np.array([2.0, 0.5]), 0.0)
        ctx.solve_fixed(np.arange(33) * 0.0625)
        ctx.smooth()
        assert np.all(ctx.get(h.F_RETCODE) == 0)
        rec = _records(ctx)
        lv = 0.03 * np.cos(np.arange(N))
        out = _check(ctx, rec, 1, 0, lv, 0, 2, "run-time compiled d=4 EK1(2) N=70, per-trajectory levels")
        assert out["count"].min() >= 1 and len(set(out["time"][0])) == N


@pytest.mark.parametrize("source", [0, 1])
def test_an_exact_hit_returns_the_stored_record(lv_fixed, source):
    ctx, rec = lv_fixed
    N, ii = 130, np.arange(130)
    keep = _bind(ctx, 1, 1.0, 0, 4)
    ref = _abi(ctx, source)
    k1 = ref["save"][1].astype(int) + 1                                                 # the second bracket (every trajectory has three)
    mean, cov = (rec["smean"], rec["scov"]) if source else (rec["mean"], rec["cov"])
    lv = mean[k1, 1, ii].copy()
    out = _check(ctx, rec, source, 1, lv, 0, 4, "exact hit")
    hit = np.argmax(out["save"] == ref["save"][1][None, :], axis=0)                     # its slot under the new level
    assert np.all(out["save"][hit, ii] == ref["save"][1]) and np.all(out["neval"][hit, ii] == 0)
    assert np.array_equal(out["time"][hit, ii], rec["t"][k1])
    assert np.array_equal(out["u"][hit, :, ii], mean[k1, :2, ii])
    assert np.array_equal(out["tvar"][hit, ii], cov[k1, 2, ii] / (mean[k1, 3, ii] * mean[k1, 3, ii]))
    del keep


def test_cache_and_invalidation(pkg):
    import torch

    h = _host()
    vf = orc.vector_field("lotka_volterra")
    N, grid = 70, np.arange(49) * 2.0 ** -4
    with pkg.Context("lotka_volterra", 2, h.EK1_ID, N) as ctx:
        ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-2)
        ctx.solve_fixed(grid)
        keep = _bind(ctx, 1, 0.8, 0, 2)
        a = _abi(ctx, 0)
        n1 = ctx.kernel_time_ms(5)[1]
        b = _abi(ctx, 0)
        assert n1 == 2 and ctx.kernel_time_ms(5)[1] == 2                              # scan + refinement once; the second request launched nothing
        assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in er.KEYS)
        ptr, nbytes = ctx.device_ptr(h.event_field(0, h.EV_TIME))                     # the device copy is the cached array
        assert nbytes == 8 * 2 * N and ctx.kernel_time_ms(5)[1] == 2
        assert ctx.field_bytes(h.event_field(0, h.EV_U)) == 8 * 2 * 2 * N and ctx.field_bytes(h.event_field(0, h.EV_COUNT)) == 4 * N
        keep2 = _bind(ctx, 1, 0.9, 0, 3)                                              # rebinding the level (and K) drops the cache
        c = _abi(ctx, 0)
        assert ctx.kernel_time_ms(5)[1] == 4 and c["time"].shape == (3, N) and not np.array_equal(c["time"][0], a["time"][0])
        ptr, nbytes = ctx.device_ptr(h.F_MEAN)                                        # a writable pointer: the cache goes ...

        class Raw:
            __cuda_array_interface__ = {"shape": (nbytes // 8,), "typestr": "<f8", "data": (ptr, False), "version": 2}

        torch.as_tensor(Raw(), device="cuda").mul_(1.25)                              # ... and the records change under it
        torch.cuda.synchronize()
        d = _abi(ctx, 0)
        assert ctx.kernel_time_ms(5)[1] == 6 and not np.array_equal(d["time"][0], c["time"][0])
        rec = _records(ctx, smoothed=False)
        er.check(rec, d, 1, 0.9, 0, 3, False, label="scaled")
        with pytest.raises(pkg.OdefError, match="needs odef_smooth first"):
            _abi(ctx, 1)
        ctx.smooth()                                                                  # new smoothed records leave source 0 alone
        e = _abi(ctx, 0)
        assert ctx.kernel_time_ms(5)[1] == 6 and np.array_equal(e["time"], d["time"], equal_nan=True)
        s1 = _abi(ctx, 1)
        assert ctx.kernel_time_ms(5)[1] == 8 and s1["time"].shape == (3, N)
        ctx.solve_fixed(grid)                                                         # a new solve: the records are the unscaled ones again
        f = _abi(ctx, 0)
        assert ctx.kernel_time_ms(5)[1] == 10 and all(np.array_equal(f[k], c[k], equal_nan=True) for k in er.KEYS)
        del keep, keep2


def test_refusals(pkg):
    h = _host()
    vf = orc.vector_field("lorenz63")
    N, grid = 3, np.arange(9) * 2.0 ** -6
    dev = lambda *a: h._to_device(a, -1)  # noqa: E731
    u0s = np.asarray(vf.u0)[None, :] * (1.0 + 1e-2 * np.random.default_rng(9).standard_normal((N, 3)))

    def bind(ctx, spec=(0, 0, 2), level=(0.5,), spec_bytes=None, level_bytes=None):
        bufs = dev(np.asarray(spec, np.int64), np.asarray(level, float))
        ctx.bind_device(h.EV_SPEC, bufs[0].data_ptr(), bufs[0].numel() * 8 if spec_bytes is None else spec_bytes)
        ctx.bind_device(h.EV_LEVEL, bufs[1].data_ptr(), bufs[1].numel() * 8 if level_bytes is None else level_bytes)
        return bufs

    with pkg.Context("lorenz63", 2, h.EK1_ID, N) as ctx:
        ctx.set_problem(u0s, vf.p, 0.0)
        keep = bind(ctx)
        with pytest.raises(pkg.OdefError, match="before a solve"):
            ctx.events(0)
        ctx.solve_fixed(grid)
        assert ctx.events(0).count.shape == (N,)
        with pytest.raises(pkg.OdefError, match="needs odef_smooth first"):
            ctx.events(1)
        ctx.bind_device(h.EV_LEVEL, 0, 0)
        with pytest.raises(pkg.OdefError, match="input missing.*ODEF_EV_LEVEL"):
            ctx.events(0)
        ctx.bind_device(h.EV_SPEC, 0, 0)
        with pytest.raises(pkg.OdefError, match="input missing.*ODEF_EV_SPEC"):
            ctx.events(0)
        keep = bind(ctx, spec=(0, 0, 2, 0), spec_bytes=32)
        with pytest.raises(pkg.OdefError, match="ODEF_EV_SPEC holds 32 bytes"):
            ctx.events(0)
        keep = bind(ctx, level=(0.5, 0.5))
        with pytest.raises(pkg.OdefError, match="ODEF_EV_LEVEL holds 16 bytes"):
            ctx.events(0)
        for spec, msg in (((3, 0, 2), r"component 3 outside 0 .. d - 1 = 2"), ((-1, 0, 2), "component -1 outside"),
                          ((0, 2, 2), r"direction 2 outside \{-1, 0, 1\}"), ((0, -2, 2), "direction -2 outside"),
                          ((0, 0, 0), "K = 0"), ((0, 0, (1 << 31) // (N * 3 * 8) + 1), "below 2 GiB"), ((0, 0, 1 << 40), "below 2 GiB")):
            keep = bind(ctx, spec=spec)
            with pytest.raises(pkg.OdefError, match=msg):
                ctx.events(0)
            with pytest.raises(pkg.OdefError, match=msg):
                ctx.field_bytes(h.event_field(0, h.EV_TIME))
        keep = bind(ctx, level=(0.5, 0.4, 0.3))
        assert ctx.events(0).t.shape == (N, 2)                                        # a refusal leaves the context usable
    with pkg.Context("lorenz63", 2, h.EK0_ID, N, diffusion="fixedMV") as ctx:
        ctx.set_problem(u0s, vf.p, 0.0)
        ctx.solve_fixed(grid)
        keep = bind(ctx)
        with pytest.raises(pkg.OdefError, match="dynamicMV / :fixedMV"):
            ctx.events(0)
    with pkg.Context("lorenz63", 2, h.EK1_ID, N, save_everystep=False) as ctx:
        ctx.set_problem(u0s, vf.p, 0.0)
        ctx.solve_fixed(grid)
        keep = bind(ctx)
        with pytest.raises(pkg.OdefError, match="kept only the final state"):
            ctx.events(0)
    with pkg.Context("lorenz63", 4, h.EK1_ID, N) as ctx:
        ctx.set_problem(u0s, vf.p, 0.0)
        ctx.solve_fixed(grid)
        keep = bind(ctx)
        with pytest.raises(pkg.OdefError, match=r"no kernel for \(d, q\) = \(3, 4\)"):
            ctx.events(0)
    l96 = orc.vector_field("lorenz96")
    with pkg.Context("lorenz96", 1, h.EK0_ID, 2) as ctx:
        ctx.set_problem(np.asarray(l96.u0)[None, :] * np.array([[1.0], [1.001]]), l96.p, 0.0)
        ctx.solve_fixed(np.arange(3) * 2.0 ** -7)
        keep = bind(ctx)
        with pytest.raises(pkg.OdefError, match=r"no kernel for \(d, q\) = \(16, 1\)"):
            ctx.events(0)
    del keep


def test_group_on_one_device_equals_the_context(pkg):
    h = _host()
    vf = orc.vector_field("lotka_volterra")
    N, grid = 131, np.arange(65) * 2.0 ** -4
    per = 1.0 + 0.02 * np.cos(np.arange(N))
    for kw in (dict(n_devices=2, device_ids=[0, 0]), dict(n_devices=1)):
        with h.DeviceGroup("lotka_volterra", 2, h.EK1_ID, N, kw["n_devices"], device_ids=kw.get("device_ids"), smooth=True) as grp, \
                pkg.Context("lotka_volterra", 2, h.EK1_ID, N, smooth=True) as ctx:
            for c in (grp, ctx):
                c.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-2)
                c.solve_fixed(grid)
                c.smooth()
            sol = pkg.EnsembleSolution(ctx, pkg.EK1(order=2, smooth=True), False)
            for level, smoothed in ((1.0, False), (per, True)):
                g = grp.events(1, level, 0, 3, smoothed=smoothed)
                s = sol.events(1, level=level, direction=0, max_events=3, smoothed=smoothed)
                assert g.count.shape == (N,) and g.t.shape == (N, 3) and g.u.shape == (N, 3, 2) and g.count.min() >= 1
                for k in ("count", "t", "t_std", "u", "direction", "save", "neval"):
                    assert getattr(g, k).tobytes() == getattr(s, k).tobytes(), k
            assert sol.events(1, level=1.0).t.tobytes() == sol.events(1, level=1.0, smoothed=True).t.tobytes()  # None: smoothed


def test_the_period_of_the_lotka_volterra_cycle(pkg):
    """The application: the period per trajectory as the difference of the 1st and 3rd located crossing of u_2 = 1 (both directions:
    they alternate), against the same difference of DOP853 events (rtol = atol = 1e-12); bound: 3 times the root sum of squares of the
    two reported standard deviations."""
    vf = orc.vector_field("lotka_volterra")
    N, scale = 16, 1e-2
    ens = pkg.EnsembleProblem(pkg.ODEProblem("lotka_volterra", vf.u0, (0.0, 6.0), vf.p), perturb_scale=scale)
    sol = pkg.solve(ens, pkg.EK1(order=3, smooth=True), pkg.EnsembleHIP(), trajectories=N, dt=2.0 ** -4, adaptive=False)
    ev = sol.events(1, level=1.0, direction=0, max_events=4)
    assert ev.t.shape == (N, 4) and ev.count.min() >= 3
    u0s = orc.ensemble_u0(vf.u0, N, scale)
    worst = 0.0
    for i in range(N):
        truth = solve_ivp(lambda t, u: vf.f(u, vf.p, t), (0.0, 6.0), u0s[i], method="DOP853", rtol=1e-12, atol=1e-12,
                          events=lambda t, u: u[1] - 1.0)
        te = truth.t_events[0]
        assert len(te) == ev.count[i], (i, len(te), ev.count[i])
        period, want = ev.t[i, 2] - ev.t[i, 0], te[2] - te[0]
        bound = 3.0 * np.hypot(ev.t_std[i, 0], ev.t_std[i, 2])
        worst = max(worst, abs(period - want) / bound)
        assert abs(period - want) <= bound, (i, period, want, bound)
    print(f"period {np.mean(ev.t[:, 2] - ev.t[:, 0]):.4f}; worst error / (3 root-sum-square standard deviations) {worst:.3f}")
