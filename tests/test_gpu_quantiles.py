"""Ensemble quantiles on the device (odef_quantile_field) against the definition in tests/_quantile_reference.py
applied to the records the same context returns.  An order statistic is an integer-counting problem and the interpolation rounds
once per operation on both sides, so every comparison is exact (assert_array_equal): no tolerance anywhere in this file."""
import numpy as np
import pytest

import _quantile_reference as qr
import odefilter_oracle as orc

pytestmark = pytest.mark.gpu

P8 = qr.PROBS8
P3 = np.array([0.95, 0.05, 0.5])
K = 6  # `which` of the pass


def _host():
    from odefilters_jl_amd import host

    return host


def _mean_records(ctx, source):
    h = _host()
    if source == 2:
        n_q = ctx.field_bytes(h.F_DENSE_MEAN) // (8 * ctx.D * ctx.N)
        return ctx.get(h.F_DENSE_MEAN).reshape(n_q, ctx.D, ctx.N)
    return ctx.get((h.F_MEAN, h.F_SMOOTH_MEAN)[source])


def _check_source(ctx, source, probs, label, expect_count=None):
    h = _host()
    got = ctx.ensemble_quantiles(source, probs)
    want = qr.reference(_mean_records(ctx, source), ctx.get(h.F_RETCODE), ctx.d, probs)
    if expect_count is not None:
        assert np.all(want[0] == expect_count), (label, want[0])
    qr.check(got, want, label=label)
    return got


def _check_launches(ctx, source, label):
    """n_launches of which = 6 is that of the last pass, and the pass ran as many digit passes as the records' key widths ask."""
    assert ctx.kernel_time_ms(K)[1] == _expected_launches(ctx, source), label


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 1001, 12289])
def test_lorenz63_filter_and_smoothed_records(pkg, N):
    h = _host()
    vf = orc.vector_field("lorenz63")
    with pkg.Context("lorenz63", 3, h.EK1_ID, N, smooth=True) as ctx:
        ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-3)
        ctx.solve_fixed(np.arange(65) * 2.0**-9)
        ctx.smooth()
        for source in (0, 1):
            n, q = _check_source(ctx, source, P8, f"lorenz63 EK1(3) N={N} source {source}", expect_count=N)
            assert n.dtype == np.int64 and n.shape == (65,) and q.shape == (65, 8, 3)
            np.testing.assert_array_equal(n, ctx.ensemble_moments(source)[0])
            ms, nl = ctx.kernel_time_ms(K)
            assert ms > 0 and nl >= 4
            _check_launches(ctx, source, f"N={N} source {source}")
            assert ctx.kernel_name(K).startswith("odef::quantile")


def test_identical_trajectories_give_that_trajectory(pkg):
    h = _host()
    vf = orc.vector_field("lorenz63")
    N = 300
    with pkg.Context("lorenz63", 3, h.EK1_ID, N, smooth=True) as ctx:
        ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 0.0)
        ctx.solve_fixed(np.arange(33) * 2.0**-9)
        ctx.smooth()
        for source in (0, 1):
            n, q = ctx.ensemble_quantiles(source, P8)
            mean = _mean_records(ctx, source)
            assert np.all(n == N)
            np.testing.assert_array_equal(mean[:, :3, :], np.repeat(mean[:, :3, :1], N, axis=2))
            np.testing.assert_array_equal(q, np.repeat(mean[:, None, :3, 0], 8, axis=1))
            assert q.tobytes() == np.repeat(mean[:, None, :3, 0], 8, axis=1).tobytes()


CASES = [
    ("fhn", 1, "EK0", "dynamic", 300, 24, 2.0**-6, 1e-3),
    ("lotka_volterra", 4, "EK0", "fixedMV", 300, 24, 2.0**-6, 1e-3),
    ("lorenz96", 2, "EK1", "dynamic", 70, 12, 2.0**-7, 1e-2),
    ("pleiades", 2, "EK1", "dynamic", 5, 12, 2.0**-10, 1e-3),
]


@pytest.mark.parametrize("name,q,kind,diffusion,N,ns,dt,scale", CASES, ids=[c[0] for c in CASES])
def test_every_kernel_family_and_d_mapping(pkg, name, q, kind, diffusion, N, ns, dt, scale):
    """d = 2 (lane kernels), d = 2 with the :fixedMV postamble, d = 16 and d = 28 (workgroup-per-trajectory kernels), P = 3.  The
    quantiles are requested before and after odef_smooth, and again after a second solve on a longer grid: every request must
    describe the records as they are then."""
    h = _host()
    vf = orc.vector_field(name)
    alg = h.EK0_ID if kind == "EK0" else h.EK1_ID
    with pkg.Context(name, q, alg, N, diffusion=diffusion, smooth=True) as ctx:
        ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, scale)
        ctx.solve_fixed(np.arange(ns + 1) * dt)
        assert np.all(ctx.get(h.F_RETCODE) == 0)
        _check_source(ctx, 0, P3, f"{name} filter, before smooth", expect_count=N)
        with pytest.raises(pkg.OdefError, match="needs odef_smooth first"):
            ctx.ensemble_quantiles(1)
        ctx.smooth()
        _check_source(ctx, 0, P3, f"{name} filter, after smooth", expect_count=N)
        _check_source(ctx, 1, P3, f"{name} smoothed", expect_count=N)
        ctx.solve_fixed(np.arange(ns + 5) * dt)
        n, qq = _check_source(ctx, 0, P3, f"{name} filter, second solve", expect_count=N)
        assert n.shape == (ns + 5,) and qq.shape == (ns + 5, 3, ctx.d)
        with pytest.raises(pkg.OdefError, match="needs odef_smooth first"):
            ctx.ensemble_quantiles(1)


def test_a_trajectory_that_did_not_succeed_is_left_out(pkg):
    vf = orc.vector_field("lorenz63")
    N = 130
    u0s = orc.ensemble_u0(vf.u0, N, 1e-3)
    u0s[77] = [1e200, 1e200, 1e200]
    prob = pkg.EnsembleProblem(pkg.ODEProblem("lorenz63", vf.u0, (0.0, 0.125), vf.p), u0s=u0s)
    with pytest.warns(RuntimeWarning):
        sol = pkg.solve(prob, pkg.EK1(order=3, smooth=False), pkg.EnsembleHIP(), dt=2.0**-6, adaptive=False)
    rc = sol.retcode_raw
    assert rc[77] == 3 and np.count_nonzero(rc) == 1
    assert np.all(np.isfinite(sol.ctx.get(0)[0, :3, 77]))  # its first record is finite: the retcode excludes it there too
    n, q = _check_source(sol.ctx, 0, P8, "lorenz63 with one Unstable trajectory", expect_count=N - 1)
    assert np.all(np.isfinite(q)) and np.all(np.abs(q) < 1e3)  # the 1e200 start is in no quantile, not even p = 1
    qq = sol.quantiles(P8)
    np.testing.assert_array_equal(qq, q)
    s = sol.summary(quantiles=(0.05, 0.95))
    np.testing.assert_array_equal(s.n, n)
    np.testing.assert_array_equal(s.qlow, q[:, 4])
    np.testing.assert_array_equal(s.med, q[:, 2])
    np.testing.assert_array_equal(s.qhigh, q[:, 0])
    assert s.quantile_probs == (0.05, 0.95)


def test_adaptive_solves_take_the_quantiles_of_their_dense_output(pkg):
    h = _host()
    vf = orc.vector_field("lorenz63")
    N, t1 = 257, 1.0
    ens = pkg.EnsembleProblem(pkg.ODEProblem("lorenz63", vf.u0, (0.0, t1), vf.p), perturb_scale=1e-3)
    sol = pkg.solve(ens, pkg.EK1(order=3), pkg.EnsembleHIP(), trajectories=N, dt=2.0**-9, adaptive=True, max_steps=512)
    assert sol.retcode == ["Success"] * N
    for source in (0, 1):
        with pytest.raises(pkg.OdefError, match="evaluate odef_dense_output at common times and use source 2"):
            sol.ctx.ensemble_quantiles(source, P8)
        with pytest.raises(pkg.OdefError, match="evaluate odef_dense_output at common times and use source 2"):
            sol.ctx.field_bytes(h.quantile_field(source, 0))
    with pytest.raises(pkg.OdefError, match="adaptive"):
        sol.quantiles(P8)
    tq = np.concatenate([[-0.25], np.linspace(0.0, t1, 9)])
    q = sol.quantiles(P8, t=tq)
    n = sol.ctx.get(h.quantile_field(2, 1))
    m, _ = sol(tq)  # [N, n_t, D]
    want = qr.reference(m.transpose(1, 2, 0), sol.retcode_raw, 3, P8)
    qr.check((n, q), want, label="adaptive dense")
    assert q.shape == (10, 8, 3) and n.tolist() == [0] + [N] * 9
    assert np.all(np.isnan(q[0])) and np.all(np.isfinite(q[1:]))
    s = sol.summary(t=tq, quantiles=(0.05, 0.95))
    np.testing.assert_array_equal(s.med, q[:, 2])
    np.testing.assert_array_equal(s.qlow, q[:, 4])
    np.testing.assert_array_equal(s.qhigh, q[:, 0])
    np.testing.assert_array_equal(s.n, n)
    np.testing.assert_array_equal(s.t, tq)
    assert s.med.shape == (10, 3) and s.quantile_probs == (0.05, 0.95)
    assert sol.summary(t=tq).med is None


def _expected_launches(ctx, source):
    """Launches of the pass over the records as they are: four per slab of 1024 / d times and two per digit pass."""
    h = _host()
    mean = _mean_records(ctx, source)
    slab = min(1024 // ctx.d, mean.shape[0])
    return 4 * -(-mean.shape[0] // slab) + 2 * qr.expected_passes(mean, ctx.get(h.F_RETCODE), ctx.d, slab)


def test_cache_rule(pkg):
    """A second request reads the cache (bit-identical, time and launch count of the pass unchanged); other probabilities, a new
    solve and a writable pointer to the mean records each make the next request compute anew.  The requests after the new solve
    and after the write leave the probabilities bound (no bind, which would drop the cache by itself), and the launch count of the
    pass is that of the NEW records: start values of 1 +- 1e-3 are 2^44 keys wide (6 digit passes), 1 +- 0.5 and a row that holds
    1234.5 more than 2^48 (7 passes), so a fresh pass shows in the count whatever the timer reads."""
    import torch

    h = _host()
    vf = orc.vector_field("lorenz63")
    N, grid, u0 = 1001, np.arange(17) * 2.0**-9, [1.0, 1.0, 1.0]
    with pkg.Context("lorenz63", 3, h.EK1_ID, N) as ctx:
        ctx.set_problem_perturbed(u0, vf.p, 0.0, 1e-3)
        ctx.solve_fixed(grid)
        n0, q0 = _check_source(ctx, 0, P3, "first request", expect_count=N)
        ms0, nl0 = ctx.kernel_time_ms(K)
        assert nl0 == _expected_launches(ctx, 0)
        for probs in (None, P3):  # bound already; bit for bit those bound: neither binds
            n1, q1 = ctx.ensemble_quantiles(0, probs)
            assert n1.tobytes() == n0.tobytes() and q1.tobytes() == q0.tobytes()
            assert ctx.kernel_time_ms(K) == (ms0, nl0)
        # the device copy is the host copy
        ptr, nbytes = ctx.device_ptr(h.quantile_field(0, 0))
        assert nbytes == q0.nbytes

        class RawQ:
            __cuda_array_interface__ = {"shape": (nbytes // 8,), "typestr": "<f8", "data": (ptr, False), "version": 2}

        assert torch.as_tensor(RawQ(), device="cuda").clone().cpu().numpy().tobytes() == q0.tobytes()
        # other probabilities
        n2, q2 = _check_source(ctx, 0, P8, "other probabilities")
        assert q2.shape == (17, 8, 3)
        np.testing.assert_array_equal(q2[:, [0, 4, 2]], q0)
        ctx.ensemble_quantiles(0, P3)
        # a new solve, the probabilities left bound
        ctx.set_problem_perturbed(u0, vf.p, 0.0, 0.5)
        ctx.solve_fixed(grid)
        n4, q4 = ctx.ensemble_quantiles(0)
        qr.check((n4, q4), qr.reference(_mean_records(ctx, 0), ctx.get(h.F_RETCODE), 3, P3), label="after a new solve")
        assert np.all(q4[0, 0] - q4[0, 1] > 0.5)  # the 5-95 % band of the new start values, not the 2e-3 of the old ones
        nl4 = ctx.kernel_time_ms(K)[1]
        assert nl4 == _expected_launches(ctx, 0) > nl0  # a pass over the NEW records: they are wider, it is longer
        # back to the narrow ensemble, then a write through a writable pointer to the records, the probabilities left bound
        ctx.set_problem_perturbed(u0, vf.p, 0.0, 1e-3)
        ctx.solve_fixed(grid)
        ctx.ensemble_quantiles(0, np.array([1.0, 0.5, 0.0]))
        assert ctx.kernel_time_ms(K)[1] == nl0
        ptr, nbytes = ctx.device_ptr(h.F_MEAN)

        class Raw:
            __cuda_array_interface__ = {"shape": (nbytes // 8,), "typestr": "<f8", "data": (ptr, False), "version": 2}

        rec = torch.as_tensor(Raw(), device="cuda").view(17, ctx.D, N)
        rec[5, 1, 333] = 1234.5
        torch.cuda.synchronize()
        n5, q5 = ctx.ensemble_quantiles(0)
        qr.check((n5, q5), qr.reference(_mean_records(ctx, 0), ctx.get(h.F_RETCODE), 3, [1.0, 0.5, 0.0]), label="after a write")
        assert q5[5, 0, 1] == 1234.5 and np.all(q5[5, 0, [0, 2]] < 100.0)
        assert ctx.kernel_time_ms(K)[1] == _expected_launches(ctx, 0) > nl0  # and again: the row with 1234.5 is wider
        # a set_problem drops the cache as well; the records are the same, so is the result, bit for bit
        ctx.set_problem_perturbed(u0, vf.p, 0.0, 1e-3)
        n6, q6 = ctx.ensemble_quantiles(0)
        assert q6.tobytes() == q5.tobytes() and n6.tobytes() == n5.tobytes()


def test_refusals(pkg):
    h = _host()
    vf = orc.vector_field("lorenz63")
    with pkg.Context("lorenz63", 3, h.EK1_ID, 8, smooth=True) as ctx:
        ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-3)
        for source in (0, 1, 2):
            with pytest.raises(pkg.OdefError, match="before a solve"):
                ctx.ensemble_quantiles(source, P3)
        ctx.solve_fixed(np.arange(9) * 2.0**-9)
        ctx.bind_quantile_probs(0, 0)
        with pytest.raises(pkg.OdefError, match="no probabilities bound"):
            ctx.ensemble_quantiles(0)
        with pytest.raises(pkg.OdefError, match="needs odef_smooth first"):
            ctx.ensemble_quantiles(1, P3)
        with pytest.raises(pkg.OdefError, match="needs odef_dense_output"):
            ctx.ensemble_quantiles(2, P3)
        buf = h._to_device((np.linspace(0.0, 1.0, 9),), ctx.cfg.device)[0]
        for P in (0, 9):
            ctx.bind_quantile_probs(buf.data_ptr(), P)
            with pytest.raises(pkg.OdefError, match="1 <= P <= 8"):
                ctx.ensemble_quantiles(0)
            with pytest.raises(pkg.OdefError, match="1 <= P <= 8"):
                ctx.field_bytes(h.quantile_field(0, 0))
        for bad in (-0.1, 1.5, np.nan):
            with pytest.raises(pkg.OdefError, match=r"outside \[0, 1\]"):
                ctx.ensemble_quantiles(0, [0.5, bad])
        for f in (h.quantile_field(0, 0), h.quantile_field(0, 1), h.quantile_field(2, 0)):
            with pytest.raises(pkg.OdefError, match="cannot be bound"):
                ctx.bind_device(f, 0, 0)
        # and after all that a good request still works
        _check_source(ctx, 0, P3, "after the refusals", expect_count=8)
        ctx.dense_output(np.array([0.0, 2.0**-10]), False)
        n, q = _check_source(ctx, 2, P3, "dense output of a fixed-grid solve", expect_count=8)
        assert q.shape == (2, 3, 3)
