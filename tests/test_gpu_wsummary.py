"""Weighted ensemble summary on the device (odef_wsummary_field) against the extended-precision reference of
tests/_wsummary_reference.py applied to the records and the log-weights the same context holds.  Bounds (derived, u = 2^-53, n =
COUNT, per time and entry, no factor on top): MEAN and COV_WITHIN 2 (n + 4) u sum_i w_i |x_i|, COV_BETWEEN 2 (n + 4) u sum_i w_i
|c_ik c_il| + beta_k beta_l, ESS 3 (n + 4) u relative, LOG_EVIDENCE (n + 8) u + 2 u |value|.  The reference prints every
error / bound ratio before it asserts."""
import numpy as np
import pytest

import _summary_reference as sr
import _wsummary_reference as wr
import odefilter_oracle as orc

pytestmark = pytest.mark.gpu
K = 7  # `which` of the pass


def _host():
    from odefilters_jl_amd import host

    return host


def _records(ctx, source):
    h = _host()
    if source == 2:
        n_q = ctx.field_bytes(h.F_DENSE_MEAN) // (8 * ctx.D * ctx.N)
        return ctx.get(h.F_DENSE_MEAN).reshape(n_q, ctx.D, ctx.N), ctx.get(h.F_DENSE_COV_TRIL).reshape(n_q, ctx.TRI, ctx.N)
    return ctx.get((h.F_MEAN, h.F_SMOOTH_MEAN)[source]), ctx.get((h.F_COV_TRIL, h.F_SMOOTH_COV_TRIL)[source])


def _check_source(ctx, source, logw, label, expect_count=None, equal=False):
    """The six arrays of `source` under `logw` against the reference; equal=True: the moments against the UNWEIGHTED reference."""
    h = _host()
    got = ctx.weighted_moments(source, logw)
    mean, cov = _records(ctx, source)
    rc = ctx.get(h.F_RETCODE)
    ref = wr.reference(mean, cov, rc, logw, ctx.d)
    if expect_count is not None:
        assert np.all(ref["count"] == expect_count), (label, ref["count"])
    values = None
    if equal:
        cnt, m, w, b, _, _ = sr.reference(mean, cov, rc, ctx.d)
        assert np.array_equal(cnt, ref["count"]) and np.array_equal(cnt, ctx.ensemble_moments(source)[0])
        values = {"mean": m, "within": w, "between": b, "log_evidence": np.full(len(cnt), logw[0], np.longdouble),
                  "ess": cnt.astype(np.longdouble)}
    worst = wr.check(got, ref, ctx.d, label=label, values=values)
    print(f"{label}: error / bound  " + "  ".join(f"{n} {r:.3g}" for n, r in zip(wr.NAMES, worst)))
    return got


def _synthetic_weights(N, seed):
    return -100.0 - 20.0 * np.random.default_rng(seed).standard_normal(N) ** 2


@pytest.mark.parametrize("N,ns", [(1, 8), (63, 8), (64, 8), (65, 8), (1001, 8), (12289, 2)])
def test_lorenz63_filter_and_smoothed_records(pkg, N, ns):
    """The weights are the data log-likelihood of noisy observations of one trajectory's own filter means, from the device."""
    h = _host()
    vf = orc.vector_field("lorenz63")
    ens = pkg.EnsembleProblem(pkg.ODEProblem("lorenz63", vf.u0, (0.0, ns * 2.0**-9), vf.p), perturb_scale=1e-3)
    sol = pkg.solve(ens, pkg.EK1(order=3), pkg.EnsembleHIP(), trajectories=N, dt=2.0**-9, adaptive=False)
    ctx = sol.ctx
    assert ctx.n_save == ns + 1 and sol.smoothed
    saves = np.arange(1, ns + 1, max(1, ns // 4))
    sigma = 1e-3
    truth = ctx.get(h.F_MEAN)[saves, :3, N // 2]
    data = truth + sigma * np.random.default_rng(N).standard_normal(truth.shape)
    logw = sol.data_loglik(sol.t[saves], data, sigma**2)[0]
    assert logw.shape == (N,) and np.all(np.isfinite(logw))
    for source in (0, 1):
        got = _check_source(ctx, source, logw, f"lorenz63 EK1(3) N={N} source {source} data log-likelihood", expect_count=N)
        n, m, w, b, le, ess = got
        assert n.dtype == np.int64 and n.shape == le.shape == ess.shape == (ns + 1,) and m.shape == (ns + 1, 3) and w.shape == b.shape == (ns + 1, 6)
        ms, nl = ctx.kernel_time_ms(K)
        assert ms > 0 and nl == 6
        assert ctx.kernel_name(K).startswith("odef::wsummary_sums_kernel<")
        _check_source(ctx, source, np.full(N, -3.5), f"lorenz63 EK1(3) N={N} source {source} equal weights", expect_count=N, equal=True)


CASES = [
    ("fhn", 1, "EK0", "dynamic", 300, 24, 2.0**-6, 1e-3),
    ("lorenz96", 2, "EK1", "dynamic", 70, 12, 2.0**-7, 1e-2),
    ("pleiades", 2, "EK1", "dynamic", 5, 2, 2.0**-10, 1e-3),
]


@pytest.mark.parametrize("name,q,kind,diffusion,N,ns,dt,scale", CASES, ids=[c[0] for c in CASES])
def test_every_kernel_family_and_d_mapping(pkg, name, q, kind, diffusion, N, ns, dt, scale):
    """d = 2 (lane kernels), d = 16 and d = 28 (workgroup-per-trajectory kernels): K = 8, 2, 1."""
    h = _host()
    vf = orc.vector_field(name)
    alg = h.EK0_ID if kind == "EK0" else h.EK1_ID
    logw = _synthetic_weights(N, ns)
    with pkg.Context(name, q, alg, N, diffusion=diffusion, smooth=True) as ctx:
        ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, scale)
        ctx.solve_fixed(np.arange(ns + 1) * dt)
        assert np.all(ctx.get(h.F_RETCODE) == 0)
        _check_source(ctx, 0, logw, f"{name} {kind}({q}) filter", expect_count=N)
        with pytest.raises(pkg.OdefError, match="needs odef_smooth first"):
            ctx.weighted_moments(1)
        ctx.smooth()
        _check_source(ctx, 1, logw, f"{name} {kind}({q}) smoothed", expect_count=N)
        _check_source(ctx, 1, np.zeros(N), f"{name} {kind}({q}) smoothed, equal weights", expect_count=N, equal=True)


def test_adaptive_solves_summarise_their_dense_output(pkg):
    h = _host()
    vf = orc.vector_field("lorenz63")
    N, t1 = 65, 0.5
    ens = pkg.EnsembleProblem(pkg.ODEProblem("lorenz63", vf.u0, (0.0, t1), vf.p), perturb_scale=1e-3)
    sol = pkg.solve(ens, pkg.EK1(order=3), pkg.EnsembleHIP(), trajectories=N, dt=2.0**-9, adaptive=True, max_steps=512)
    assert sol.retcode == ["Success"] * N
    logw = _synthetic_weights(N, 3)
    for source in (0, 1):
        with pytest.raises(pkg.OdefError, match="evaluate odef_dense_output at common times and use source 2"):
            sol.ctx.weighted_moments(source, logw)
        with pytest.raises(pkg.OdefError, match="evaluate odef_dense_output at common times and use source 2"):
            sol.ctx.field_bytes(h.wsummary_field(source, h.W_ESS))
    with pytest.raises(pkg.OdefError, match="adaptive"):
        sol.summary(log_weights=logw)
    tq = np.linspace(0.0, t1, 4)
    s = sol.summary(t=tq, log_weights=logw)
    _check_source(sol.ctx, 2, logw, "adaptive lorenz63, dense output at 4 common times", expect_count=N)
    got = sol.ctx.weighted_moments(2)
    il3 = np.tril_indices(3)
    assert s.n.tobytes() == got[0].tobytes() and s.mean.tobytes() == got[1].tobytes()
    assert s.cov_within[:, il3[0], il3[1]].tobytes() == got[2].tobytes() and s.cov_between[:, il3[0], il3[1]].tobytes() == got[3].tobytes()
    assert s.log_evidence.tobytes() == got[4].tobytes() and s.ess.tobytes() == got[5].tobytes()
    np.testing.assert_array_equal(s.t, tq)
    assert sol.summary(t=tq).ess is None and sol.summary(t=tq).log_evidence is None


def test_a_trajectory_that_did_not_succeed_and_a_nan_weight_are_left_out(pkg):
    vf = orc.vector_field("lorenz63")
    N = 130
    u0s = orc.ensemble_u0(vf.u0, N, 1e-3)
    u0s[77] = [1e200, 1e200, 1e200]
    prob = pkg.EnsembleProblem(pkg.ODEProblem("lorenz63", vf.u0, (0.0, 0.125), vf.p), u0s=u0s)
    with pytest.warns(RuntimeWarning):
        sol = pkg.solve(prob, pkg.EK1(order=3, smooth=False), pkg.EnsembleHIP(), dt=2.0**-6, adaptive=False)
    rc = sol.retcode_raw
    assert rc[77] == 3 and np.count_nonzero(rc) == 1
    logw = _synthetic_weights(N, 4)
    logw[77] = 1e3  # the largest log-weight belongs to the trajectory that did not succeed: it is not the shift
    got = _check_source(sol.ctx, 0, logw, "one Unstable trajectory", expect_count=N - 1)
    assert np.all(np.isfinite(got[1])) and np.all(got[4] < 0.0)
    logw[5] = np.nan
    logw[64] = np.inf
    got = _check_source(sol.ctx, 0, logw, "one Unstable trajectory, a NaN and an inf weight", expect_count=N - 3)
    s = sol.summary(log_weights=logw)
    assert np.all(s.n == N - 3) and np.all(np.isfinite(s.mean)) and np.all(np.isfinite(s.cov)) and np.all(np.isfinite(s.ess))


def test_cache_rule(pkg):
    """A second request reads the cache (bit-identical, time and launch count of the pass untouched), also when the same bits are
    handed in again; other weights, a writable pointer to the records and a new solve each make the next request compute anew."""
    import torch

    h = _host()
    vf = orc.vector_field("lorenz63")
    N, grid = 1001, np.arange(9) * 2.0**-9
    logw = _synthetic_weights(N, 5)
    with pkg.Context("lorenz63", 3, h.EK1_ID, N) as ctx:
        ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-3)
        ctx.solve_fixed(grid)
        first = _check_source(ctx, 0, logw, "first request", expect_count=N)
        # The witness that no pass ran is the TIME of the last pass: n_launches is 6 after every pass, but the event timer of a
        # new pass never reads the same float twice, so an unchanged (ms, n_launches) pair means the cache answered.
        stamp = ctx.kernel_time_ms(K)
        for w in (None, logw, logw.copy(), torch.from_numpy(logw)):  # bound already; bit for bit those bound: neither binds
            again = ctx.weighted_moments(0, w)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
            assert ctx.kernel_time_ms(K) == stamp
        for qty, want in enumerate(first):  # the device copy is the host copy
            ptr, nbytes = ctx.device_ptr(h.wsummary_field(0, qty))
            assert nbytes == want.nbytes

            class Raw:
                __cuda_array_interface__ = {"shape": (nbytes // 8,), "typestr": "<i8" if qty == 0 else "<f8", "data": (ptr, False),
                                            "version": 2}

            assert torch.as_tensor(Raw(), device="cuda").clone().cpu().numpy().tobytes() == want.tobytes()
        assert ctx.kernel_time_ms(K) == stamp
        # binding the same weights again drops the cache: the pass runs anew and agrees bit for bit
        ctx.bind_log_weights(ctx._log_weight_buf.data_ptr(), N)
        second = ctx.weighted_moments(0)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
        # other weights change the result
        other = _check_source(ctx, 0, logw[::-1].copy(), "other weights", expect_count=N)
        assert not np.array_equal(other[1], first[1]) and not np.array_equal(other[3], first[3])
        # a write through a writable pointer to the records reaches the next request, the weights left bound
        ctx.weighted_moments(0, logw)
        ptr, nbytes = ctx.device_ptr(h.F_MEAN)

        class RawMean:
            __cuda_array_interface__ = {"shape": (nbytes // 8,), "typestr": "<f8", "data": (ptr, False), "version": 2}

        torch.as_tensor(RawMean(), device="cuda").mul_(2.0)
        torch.cuda.synchronize()
        n1, m1, w1, b1, le1, ess1 = ctx.weighted_moments(0)
        assert m1.tobytes() == (2.0 * first[1]).tobytes() and b1.tobytes() == (4.0 * first[3]).tobytes()
        assert w1.tobytes() == first[2].tobytes() and le1.tobytes() == first[4].tobytes() and ess1.tobytes() == first[5].tobytes()
        # a new solve drops the cache
        ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 0.5)
        ctx.solve_fixed(grid)
        wide = _check_source(ctx, 0, logw, "after a new solve", expect_count=N)
        assert np.all(wide[3][0, [0, 2, 5]] > 100.0 * first[3][0, [0, 2, 5]])  # the spread of the new start values
        with pytest.raises(pkg.OdefError, match="cannot be bound"):
            ctx.bind_device(h.wsummary_field(0, 1), 0, 0)


def test_posterior_predictive_on_a_parameter_sweep(pkg):
    """65 candidates of Lorenz-63's rho swept around 28; the data are noisy observations of the candidate at 28 itself."""
    vf = orc.vector_field("lorenz63")
    N, sigma, true_index = 65, 1e-2, 40
    ps = np.tile(vf.p, (N, 1))
    which = int(np.argmin(np.abs(np.asarray(vf.p, float) - 28.0)))
    ps[:, which] = 28.0 + 0.05 * (np.arange(N) - true_index)
    grid = np.arange(65) * 2.0**-7
    prob = pkg.EnsembleProblem(pkg.ODEProblem("lorenz63", vf.u0, (0.0, float(grid[-1])), vf.p), u0s=np.tile(vf.u0, (N, 1)), ps=ps)
    sol = pkg.solve(prob, pkg.EK1(order=3), pkg.EnsembleHIP(), tstops=grid, adaptive=False)
    obs = np.arange(8, 65, 8)
    data = sol.ctx.get(0)[obs, :3, true_index] + sigma * np.random.default_rng(7).standard_normal((len(obs), 3))
    log_prior = -0.5 * ((ps[:, which] - 28.0) / 2.0) ** 2
    post = sol.posterior_predictive(grid[obs], data, sigma**2, log_prior=log_prior)
    loglik = sol.data_loglik(grid[obs], data, sigma**2)[0]
    assert int(np.argmax(loglik + log_prior)) == true_index
    same = sol.summary(log_weights=loglik + log_prior)
    for name in ("n", "mean", "cov_within", "cov_between", "ess", "log_evidence"):
        assert getattr(post, name).tobytes() == getattr(same, name).tobytes(), name
    assert np.all(post.n == N) and np.all(post.ess >= 1.0) and np.all(post.ess <= N) and np.all(np.isfinite(post.log_evidence))
    print(f"posterior predictive: ESS {post.ess[0]:.3f} of {N}, log evidence {post.log_evidence[0]:.3f}")
    plain = sol.summary()
    assert plain.ess is None and not np.array_equal(plain.mean, post.mean)
    with pytest.raises(pkg.OdefError, match="weighted quantiles are not built"):
        sol.summary(quantiles=(0.05, 0.95), log_weights=loglik)


def test_two_shards_pool_to_the_one_context_result(pkg):
    h = _host()
    vf = orc.vector_field("lorenz63")
    N, grid = 1001, np.arange(9) * 2.0**-9
    logw = _synthetic_weights(N, 6)
    with h.DeviceGroup("lorenz63", 3, 1, N, 2, device_ids=[0, 0], smooth=True) as grp:
        assert grp.shard(0) == (0, 501) and grp.shard(1) == (501, 500)
        grp.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-3)
        grp.solve_fixed(grid)
        grp.smooth()
        pooled = [grp.weighted_moments(source, logw) for source in (0, 1)]
    with pkg.Context("lorenz63", 3, 1, N, smooth=True) as ctx:
        ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-3)
        ctx.solve_fixed(grid)
        ctx.smooth()
        for source in (0, 1):
            mean, cov = _records(ctx, source)
            ref = wr.reference(mean, cov, ctx.get(h.F_RETCODE), logw, 3)
            assert np.all(ref["count"] == N)
            worst = wr.check(pooled[source], ref, 3, label=f"two shards, source {source}")
            print(f"two shards source {source}: error / bound  " + "  ".join(f"{n} {r:.3g}" for n, r in zip(wr.NAMES, worst)))
            _check_source(ctx, source, logw, f"one context of 1001, source {source}", expect_count=N)


def test_refusals(pkg):
    import torch

    h = _host()
    vf = orc.vector_field("lorenz63")
    N = 8
    with pkg.Context("lorenz63", 3, h.EK1_ID, N) as ctx:
        ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-3)
        buf = torch.zeros(N + 1, dtype=torch.float64, device="cuda")
        for source in (0, 1, 2):
            with pytest.raises(pkg.OdefError, match="before a solve"):
                ctx.weighted_moments(source, np.zeros(N))
        ctx.solve_fixed(np.arange(9) * 2.0**-9)
        ctx.bind_log_weights(0, N)  # NULL lets them go
        with pytest.raises(pkg.OdefError, match="no weights bound"):
            ctx.weighted_moments(0)
        with pytest.raises(pkg.OdefError, match="ODEF_W_LOGWEIGHT is double \\[N\\]"):
            ctx.bind_log_weights(buf.data_ptr(), N + 1)
        with pytest.raises(pkg.OdefError, match="no weights bound"):  # the refused bind bound nothing
            ctx.field_bytes(h.wsummary_field(0, h.W_MEAN))
        with pytest.raises(pkg.OdefError, match="values for 8 trajectories"):
            ctx.weighted_moments(0, np.zeros(N + 1))
        with pytest.raises(pkg.OdefError, match="cannot be bound"):
            ctx.bind_device(h.wsummary_field(0, h.W_ESS), buf.data_ptr(), 8 * 9)
        with pytest.raises(pkg.OdefError, match="needs odef_dense_output"):
            ctx.weighted_moments(2, np.zeros(N))
        with pytest.raises(pkg.OdefError, match="needs odef_smooth first"):
            ctx.weighted_moments(1)
        got = ctx.weighted_moments(0)  # a refusal leaves the context usable
        assert np.all(got[0] == N) and np.allclose(got[5], N) and np.allclose(got[4], 0.0)
