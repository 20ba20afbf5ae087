"""Ensemble summary on the device (odef_summary_field) against the extended-precision reference of
tests/_summary_reference.py applied to the records the same context returns.  Tolerances (derived, u = 2^-53, n = COUNT, per
time and entry): MEAN (n + 2) u mean_i|mu_ik|, COV_WITHIN (n + 2) u mean_i|Sigma_i,kl|, COV_BETWEEN n u sqrt(B_kk B_ll) and exactly 0
for n = 1.  Every test prints its worst error / bound ratios before it returns."""
import numpy as np
import pytest

import _summary_reference as sr
import odefilter_oracle as orc

pytestmark = pytest.mark.gpu


def _host():
    from odefilters_jl_amd import host

    return host


def _records(ctx, source):
    h = _host()
    if source == 2:
        n_q = ctx.field_bytes(h.F_DENSE_MEAN) // (8 * ctx.D * ctx.N)
        return ctx.get(h.F_DENSE_MEAN).reshape(n_q, ctx.D, ctx.N), ctx.get(h.F_DENSE_COV_TRIL).reshape(n_q, ctx.TRI, ctx.N)
    return ctx.get((h.F_MEAN, h.F_SMOOTH_MEAN)[source]), ctx.get((h.F_COV_TRIL, h.F_SMOOTH_COV_TRIL)[source])


def _check_source(ctx, source, label, expect_count=None):
    h = _host()
    got = ctx.ensemble_moments(source)
    mean, cov = _records(ctx, source)
    ref = sr.reference(mean, cov, ctx.get(h.F_RETCODE), ctx.d)
    if expect_count is not None:
        assert np.all(ref[0] == expect_count), (label, ref[0])
    worst = sr.check(got, ref, ctx.d, label=label)
    print(f"{label}: error / bound  MEAN {worst[0]:.3g}  COV_WITHIN {worst[1]:.3g}  COV_BETWEEN {worst[2]:.3g}")
    return got


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1001, 12289])
def test_lorenz63_filter_and_smoothed_records(pkg, N):
    h = _host()
    vf = orc.vector_field("lorenz63")
    with pkg.Context("lorenz63", 3, h.EK1_ID, N, smooth=True) as ctx:
        ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-3)
        ctx.solve_fixed(np.arange(65) * 2.0**-9)
        ctx.smooth()
        for source in (0, 1):
            n, m, w, b = _check_source(ctx, source, f"lorenz63 EK1(3) N={N} source {source}", expect_count=N)
            assert n.dtype == np.int64 and n.shape == (65,) and m.shape == (65, 3) and w.shape == b.shape == (65, 6)
        ms, nl = ctx.kernel_time_ms(2)
        assert ms > 0 and nl == 4
        assert ctx.kernel_name(2).startswith("odef::summary_sums_kernel<")


CASES = [
    ("fhn", 1, "EK0", "dynamic", 300, 24, 2.0**-6, 1e-3),
    ("lotka_volterra", 4, "EK0", "fixedMV", 300, 24, 2.0**-6, 1e-3),
    ("lorenz96", 2, "EK1", "dynamic", 70, 12, 2.0**-7, 1e-2),
    ("pleiades", 2, "EK1", "dynamic", 5, 12, 2.0**-10, 1e-3),
]


@pytest.mark.parametrize("name,q,kind,diffusion,N,ns,dt,scale", CASES, ids=[c[0] for c in CASES])
def test_every_kernel_family_and_d_mapping(pkg, name, q, kind, diffusion, N, ns, dt, scale):
    """d = 2 (lane kernels), d = 2 with the :fixedMV postamble, d = 16 and d = 28 (workgroup-per-trajectory kernels).  The summary
    is requested before and after odef_smooth, and again after a second solve on a longer grid: every request must describe the
    records as they are then."""
    h = _host()
    vf = orc.vector_field(name)
    alg = h.EK0_ID if kind == "EK0" else h.EK1_ID
    with pkg.Context(name, q, alg, N, diffusion=diffusion, smooth=True) as ctx:
        ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, scale)
        ctx.solve_fixed(np.arange(ns + 1) * dt)
        assert np.all(ctx.get(h.F_RETCODE) == 0)
        _check_source(ctx, 0, f"{name} {kind}({q}) {diffusion} filter, before smooth", expect_count=N)
        with pytest.raises(pkg.OdefError, match="needs odef_smooth first"):
            ctx.ensemble_moments(1)
        ctx.smooth()
        _check_source(ctx, 0, f"{name} {kind}({q}) {diffusion} filter, after smooth", expect_count=N)
        _check_source(ctx, 1, f"{name} {kind}({q}) {diffusion} smoothed", expect_count=N)
        ctx.solve_fixed(np.arange(ns + 5) * dt)
        got = _check_source(ctx, 0, f"{name} {kind}({q}) {diffusion} filter, second solve", expect_count=N)
        assert got[0].shape == (ns + 5,)
        with pytest.raises(pkg.OdefError, match="needs odef_smooth first"):
            ctx.ensemble_moments(1)


def test_adaptive_solves_summarise_their_dense_output(pkg):
    h = _host()
    vf = orc.vector_field("lorenz63")
    N, t1 = 257, 1.0
    ens = pkg.EnsembleProblem(pkg.ODEProblem("lorenz63", vf.u0, (0.0, t1), vf.p), perturb_scale=1e-3)
    sol = pkg.solve(ens, pkg.EK1(order=3), pkg.EnsembleHIP(), trajectories=N, dt=2.0**-9, adaptive=True, max_steps=512)
    assert sol.retcode == ["Success"] * N
    with pytest.raises(pkg.OdefError, match="before any|needs odef_dense_output"):
        sol.ctx.ensemble_moments(2)
    for source in (0, 1):
        with pytest.raises(pkg.OdefError, match="evaluate odef_dense_output at common times and use source 2"):
            sol.ctx.ensemble_moments(source)
        with pytest.raises(pkg.OdefError, match="evaluate odef_dense_output at common times and use source 2"):
            sol.ctx.field_bytes(h.summary_field(source, h.S_MEAN))
    with pytest.raises(pkg.OdefError, match="adaptive"):
        sol.summary()
    tq = np.concatenate([[-0.25], np.linspace(0.0, t1, 9)])
    s = sol.summary(t=tq)
    m, c = sol(tq)  # [N, n_t, D], [N, n_t, D, D]
    il = np.tril_indices(sol.D)
    ref = sr.reference(m.transpose(1, 2, 0), c[:, :, il[0], il[1]].transpose(1, 2, 0), sol.retcode_raw, 3)
    il3 = np.tril_indices(3)
    worst = sr.check((s.n, s.mean, s.cov_within[:, il3[0], il3[1]], s.cov_between[:, il3[0], il3[1]]), ref, 3, label="adaptive")
    print(f"adaptive lorenz63 dense: error / bound  MEAN {worst[0]:.3g}  COV_WITHIN {worst[1]:.3g}  COV_BETWEEN {worst[2]:.3g}")
    assert s.n.tolist() == [0] + [N] * 9
    assert np.all(np.isnan(s.mean[0])) and np.all(np.isnan(s.cov[0])) and np.all(np.isfinite(s.mean[1:])) and np.all(np.isfinite(s.cov[1:]))
    np.testing.assert_array_equal(s.t, tq)
    np.testing.assert_array_equal(s.cov, s.cov_within + s.cov_between)


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
    _check_source(sol.ctx, 0, "lorenz63 with one Unstable trajectory", expect_count=N - 1)
    s = sol.summary()
    assert np.all(s.n == N - 1) and np.all(np.isfinite(s.mean)) and np.all(np.isfinite(s.cov))


def test_two_requests_agree_bit_for_bit_and_the_device_copy_equals_the_host_copy(pkg):
    import torch

    h = _host()
    vf = orc.vector_field("lorenz63")
    N = 12289
    with pkg.Context("lorenz63", 3, h.EK1_ID, N) as ctx:
        ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-3)
        ctx.solve_fixed(np.arange(65) * 2.0**-9)
        first = ctx.ensemble_moments(0)
        ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-3)  # invalidates the cache; the records are the same
        second = ctx.ensemble_moments(0)
        for a, b in zip(first, second):
            assert a.tobytes() == b.tobytes()
        for qty, want in enumerate(second):
            ptr, nbytes = ctx.device_ptr(h.summary_field(0, qty))
            assert nbytes == want.nbytes

            class Raw:
                __cuda_array_interface__ = {"shape": (nbytes // 8,), "typestr": "<i8" if qty == 0 else "<f8", "data": (ptr, False),
                                            "version": 2}

            dev = torch.as_tensor(Raw(), device="cuda").clone().cpu().numpy()
            assert dev.tobytes() == want.tobytes()
        with pytest.raises(pkg.OdefError, match="cannot be bound"):
            ctx.bind_device(h.summary_field(0, 1), 0, 0)


def test_records_edited_through_their_device_pointer_reach_the_next_summary(pkg):
    """odef_get_device hands out a writable pointer, so it drops what is derived from that record set (include/odefilter.h,
    "Derived outputs and their caches").  N = 70: one full and one partial wavefront.  Scaling by a power of two is exact and the
    summation order is fixed, so MEAN doubles and COV_BETWEEN quadruples bit for bit; COV_WITHIN reads the covariances only."""
    import torch

    h = _host()
    vf = orc.vector_field("lorenz63")
    N = 70
    with pkg.Context("lorenz63", 2, h.EK1_ID, N) as ctx:
        ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-3)
        ctx.solve_fixed(np.arange(9) * 2.0**-6)
        n0, m0, w0, b0 = ctx.ensemble_moments(0)
        assert np.all(n0 == N) and np.all(np.isfinite(m0)) and np.any(m0 != 0)
        ptr, nbytes = ctx.device_ptr(h.F_MEAN)

        class Raw:
            __cuda_array_interface__ = {"shape": (nbytes // 8,), "typestr": "<f8", "data": (ptr, False), "version": 2}

        torch.as_tensor(Raw(), device="cuda").mul_(2.0)
        torch.cuda.synchronize()
        n1, m1, w1, b1 = ctx.ensemble_moments(0)
        assert n1.tobytes() == n0.tobytes()
        assert m1.tobytes() == (2.0 * m0).tobytes()
        assert b1.tobytes() == (4.0 * b0).tobytes()
        assert w1.tobytes() == w0.tobytes()


def test_two_shards_merge_to_the_one_context_summary(pkg):
    h = _host()
    vf = orc.vector_field("lorenz63")
    N, grid = 1001, np.arange(33) * 2.0**-9
    with h.DeviceGroup("lorenz63", 3, 1, N, 2, device_ids=[0, 0], smooth=True) as grp:
        assert grp.shard(0) == (0, 501) and grp.shard(1) == (501, 500)
        grp.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-3)
        grp.solve_fixed(grid)
        grp.smooth()
        merged = [grp.ensemble_moments(source) for source in (0, 1)]
        s = grp.summary(smoothed=True)
    with pkg.Context("lorenz63", 3, 1, N, smooth=True) as ctx:
        ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-3)
        ctx.solve_fixed(grid)
        ctx.smooth()
        for source in (0, 1):
            mean, cov = _records(ctx, source)
            ref = sr.reference(mean, cov, ctx.get(h.F_RETCODE), 3)
            assert np.all(ref[0] == N)
            worst = sr.check(merged[source], ref, 3, label=f"two shards, source {source}")
            print(f"two shards source {source}: error / bound  MEAN {worst[0]:.3g}  COV_WITHIN {worst[1]:.3g}  COV_BETWEEN {worst[2]:.3g}")
            _check_source(ctx, source, f"one context of 1001, source {source}", expect_count=N)
    np.testing.assert_array_equal(s.t, grid)
    np.testing.assert_array_equal(s.mean, merged[1][1])


def test_final_save_mode_summarises_the_one_record(pkg):
    h = _host()
    vf = orc.vector_field("lorenz63")
    N = 1001
    ens = pkg.EnsembleProblem(pkg.ODEProblem("lorenz63", vf.u0, (0.0, 64 * 2.0**-9), vf.p), perturb_scale=1e-3)
    sol = pkg.solve(ens, pkg.EK1(order=3, smooth=False), pkg.EnsembleHIP(), trajectories=N, dt=2.0**-9, adaptive=False,
                    save_everystep=False)
    assert sol.ctx.n_save == 1
    s = sol.summary()
    assert s.n.tolist() == [N] and s.mean.shape == (1, 3) and s.t.tolist() == [64 * 2.0**-9]
    fm = sol.final_mean()                       # [N, D]
    fc = sol.x_filt_cov()[:, 0]                 # [N, D, D]
    il = np.tril_indices(sol.D)
    ref = sr.reference(fm.T[None], fc[:, il[0], il[1]].T[None], sol.retcode_raw, 3)
    il3 = np.tril_indices(3)
    worst = sr.check((s.n, s.mean, s.cov_within[:, il3[0], il3[1]], s.cov_between[:, il3[0], il3[1]]), ref, 3, label="final")
    print(f"final save mode: error / bound  MEAN {worst[0]:.3g}  COV_WITHIN {worst[1]:.3g}  COV_BETWEEN {worst[2]:.3g}")


def test_summary_before_a_solve_is_refused(pkg):
    h = _host()
    vf = orc.vector_field("lorenz63")
    with pkg.Context("lorenz63", 3, h.EK1_ID, 8) as ctx:
        ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-3)
        for source in (0, 1, 2):
            with pytest.raises(pkg.OdefError, match="before a solve"):
                ctx.ensemble_moments(source)
        ctx.solve_fixed(np.arange(9) * 2.0**-9)
        with pytest.raises(pkg.OdefError, match="needs odef_dense_output"):
            ctx.ensemble_moments(2)
        ctx.dense_output(np.array([0.0, 2.0**-10]), False)
        _check_source(ctx, 2, "dense output of a fixed-grid solve", expect_count=8)
