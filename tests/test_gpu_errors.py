"""Per-trajectory solution errors on the device (odef_errors_field) against the extended-precision reference of
tests/_errors_reference.py applied to the records the same context returns.  Tolerances: 16 times the measured error of the
numpy float64 evaluation (`_errors_reference.C_NUMPY`), in units of the bounds derived in `unit_bounds`.  Every test prints its
worst error / unit bound ratios before it returns."""
import numpy as np
import pytest

import _errors_reference as er
from _errors_reference import orc

pytestmark = pytest.mark.gpu

KMAP = {"final": "final", "l2": "l2", "linf": "l∞", "chi2": "chi2"}


def _host():
    from odefilters_jl_amd import host

    return host


def _records(ctx, source, adaptive):
    h = _host()
    mean, cov = ctx.get((h.F_MEAN, h.F_SMOOTH_MEAN)[source]), ctx.get((h.F_COV_TRIL, h.F_SMOOTH_COV_TRIL)[source])
    ts = ctx.get(h.F_T).reshape(ctx.n_save, ctx.N) if adaptive else None
    ns = ctx.get(h.F_NSAVED) if adaptive else None
    return mean, cov, ts, ns


def _got(ctx, source):
    e = ctx.solution_errors(source)
    assert e["nused"].dtype == np.int64 and all(e[KMAP[k]].shape == (ctx.N,) for k in er.KEYS)
    return {k: e[KMAP[k]] for k in er.KEYS} | {"nused": e["nused"]}


def _check(ctx, source, truth, adaptive, label):
    mean, cov, ts, ns = _records(ctx, source, adaptive)
    ref = er.evaluate(mean, cov, ctx.d, truth, ts, ns)
    got = _got(ctx, source)
    r = er.check(got, ref, er.unit_bounds(mean, cov, ctx.d, truth, ref, ts, ns), label=label)
    print(f"{label}: error / unit bound", {k: f"{v:.3g}" for k, v in r.items()})
    return got, ref


def _u0s(N, d, base, seed):
    return np.asarray(base)[None, :] * (1.0 + 1e-2 * np.random.default_rng(seed).standard_normal((N, d)))


@pytest.mark.parametrize("adaptive", [False, True], ids=["fixed", "adaptive"])
@pytest.mark.parametrize("q", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", ["EK0", "EK1"])
def test_linear_against_its_analytic_solution(pkg, kind, q, adaptive):
    """u' = p u with u* = u0 exp(p t) from RhsLinear::analytic in the kernel; 130 trajectories (not a multiple of 64), filter and
    smoothed records.  Adaptive: NUSED = accepted steps + 1, the zero-length repeats of rejected attempts are skipped."""
    h = _host()
    vf = orc.vector_field("linear")
    N = 130
    u0s = _u0s(N, 2, vf.u0, 10 * q + adaptive)
    with pkg.Context("linear", q, h.EK0_ID if kind == "EK0" else h.EK1_ID, N, smooth=True) as ctx:
        ctx.set_problem(u0s, vf.p, 0.0)
        if adaptive:
            ctx.solve_adaptive(1.0, abstol=1e-7, reltol=1e-5, dt0=1.0, max_steps=2048)  # (the first attempt, the whole span, is rejected)
        else:
            ctx.solve_fixed(np.arange(41) * 2.0 ** -5)
        assert np.all(ctx.get(h.F_RETCODE) == 0)
        t = ctx.get(h.F_T).reshape(ctx.n_save, N) if adaptive else ctx.get(h.F_T)
        truth = er.linear_truth(u0s, vf.p, t)
        got, ref = _check(ctx, 0, truth, adaptive, f"linear {kind}({q}) {'adaptive' if adaptive else 'fixed'} filter")
        with pytest.raises(pkg.OdefError, match="need odef_smooth first"):
            ctx.solution_errors(1)
        ctx.smooth()
        _check(ctx, 1, truth, adaptive, f"linear {kind}({q}) {'adaptive' if adaptive else 'fixed'} smoothed")
        if adaptive:
            acc, rej = ctx.get(h.F_NACCEPT), ctx.get(h.F_NREJECT)
            assert np.array_equal(got["nused"], acc.astype(np.int64) + 1)
            assert rej.sum() > 0 and np.array_equal(ctx.get(h.F_NSAVED), acc + rej + 1)
        else:
            assert np.all(got["nused"] == 41)
        assert np.all(got["chi2"] > 0) and np.all(got["l2"] > 0) and np.all(got["linf"] >= got["l2"])
        ms, nl = ctx.kernel_time_ms(3)
        assert ms > 0 and nl == 2
        assert ctx.kernel_name(3) == "odef::errors_partial_kernel<2, odef::TruthAnalytic<odef::RhsLinear>>"
        # U_ANALYTIC, computed when asked for
        ua = ctx.get(h.errors_field(0, h.E_U_ANALYTIC))
        assert ua.shape == (ctx.n_save, 2, N)
        live = np.ones((ctx.n_save, N), bool) if not adaptive else np.arange(ctx.n_save)[:, None] < ctx.get(h.F_NSAVED)[None, :]
        m = np.broadcast_to(live[:, None, :], ua.shape)
        assert np.all(np.abs(ua[m] - truth[m].astype(float)) <= 4 * er.U * np.abs(truth[m].astype(float)))
        assert np.all(ua[~m] == 0.0)


def test_requests_repeat_bit_for_bit_and_follow_a_new_solve(pkg):
    h = _host()
    vf = orc.vector_field("linear")
    N = 1000
    with pkg.Context("linear", 3, h.EK1_ID, N, smooth=True) as ctx, pkg.Context("linear", 3, h.EK1_ID, N, smooth=True) as ctx2:
        with pytest.raises(pkg.OdefError, match="before a solve"):
            ctx.solution_errors(0)
        for c in (ctx, ctx2):
            c.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-2)
            c.solve_fixed(np.arange(130) * 2.0 ** -7)
        a, b, c2 = _got(ctx, 0), _got(ctx, 0), _got(ctx2, 0)
        for k in a:
            np.testing.assert_array_equal(a[k], b[k])     # the cache
            np.testing.assert_array_equal(a[k], c2[k])    # a second pass over equal records
        assert ctx.kernel_time_ms(3)[1] == 2
        ctx.solve_fixed(np.arange(70) * 2.0 ** -6)         # the cache follows the records
        t = ctx.get(h.F_T)
        u0s = ctx.get(h.F_U0).T
        got, _ = _check(ctx, 0, er.linear_truth(u0s, vf.p, t), False, "after a second solve")
        assert np.all(got["nused"] == 70) and not np.array_equal(got["l2"], a["l2"])
        ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 2e-2)   # new initial values: the truth changes, the cache goes
        assert not np.array_equal(_got(ctx, 0)["l2"], got["l2"])


def test_records_edited_through_their_device_pointer_reach_the_next_errors(pkg):
    """odef_get_device hands out a writable pointer, so it drops what is derived from that record set (include/odefilter.h,
    "Derived outputs and their caches"): after F_MEAN is doubled in place the next request runs the pass again, on the records as
    they are now.  (n_launches of this pass is set per pass, not counted up: that the pass ran anew shows in the values.)"""
    import torch

    h = _host()
    vf = orc.vector_field("linear")
    N = 70
    u0s = _u0s(N, 2, vf.u0, 7)
    with pkg.Context("linear", 2, h.EK0_ID, N) as ctx:
        ctx.set_problem(u0s, vf.p, 0.0)
        ctx.solve_fixed(np.arange(9) * 2.0 ** -6)
        truth = er.linear_truth(u0s, vf.p, ctx.get(h.F_T))
        first, _ = _check(ctx, 0, truth, False, "before the edit")
        ptr, nbytes = ctx.device_ptr(h.F_MEAN)

        class Raw:
            __cuda_array_interface__ = {"shape": (nbytes // 8,), "typestr": "<f8", "data": (ptr, False), "version": 2}

        torch.as_tensor(Raw(), device="cuda").mul_(2.0)
        torch.cuda.synchronize()
        second, _ = _check(ctx, 0, truth, False, "F_MEAN doubled")  # the reference reads the records back: the doubled ones
        ms, nl = ctx.kernel_time_ms(3)
        assert ms > 0 and nl == 2
        for k in er.KEYS:
            assert not np.array_equal(second[k], first[k]), k
        assert np.array_equal(second["nused"], first["nused"])


DECAY = """
struct NAME {
  static constexpr int d = 1, np = 1;
  template <class T>
  __device__ static void f(const T (&u)[1], const double* p, T (&du)[1]) { du[0] = -p[0] * u[0]; }
ANALYTIC
};
"""
DECAY_ANALYTIC = """  template <class T>
  __device__ static void analytic(const T (&u0)[1], const double* p, T t, T (&out)[1]) { out[0] = u0[0] * exp(-p[0] * t); }"""


def test_run_time_compiled_field_with_and_without_analytic(pkg):
    h = _host()
    pkg.compile_rhs("ErrDecay", DECAY.replace("NAME", "ErrDecay").replace("ANALYTIC", DECAY_ANALYTIC), 1, 1)
    pkg.compile_rhs("ErrDecayPlain", DECAY.replace("NAME", "ErrDecayPlain").replace("ANALYTIC", ""), 1, 1)
    N, p = 70, np.array([0.7])
    u0s = _u0s(N, 1, [1.5], 5)
    ens = pkg.EnsembleProblem(pkg.ODEProblem("ErrDecay", u0s[0], (0.0, 1.0), p), u0s=u0s)
    sol = pkg.solve(ens, pkg.EK1(order=2), pkg.EnsembleHIP(), dt=2.0 ** -5, adaptive=False)
    assert sol.smoothed
    truth = (u0s.T[None, :, :] * np.exp(-np.longdouble(p[0]) * sol.t.astype(np.longdouble))[:, None, None])
    for source in (0, 1):
        _check(sol.ctx, source, truth, False, f"run-time field, source {source}")
    e = sol.errors
    assert set(e) == {"l∞", "l2", "final", "chi2"} and all(v.shape == (N,) for v in e.values())
    np.testing.assert_array_equal(e["l2"], sol.ctx.solution_errors(1)["l2"])
    assert sol.u_analytic.shape == sol.u.shape
    np.testing.assert_allclose(sol.u_analytic, truth.astype(float).transpose(2, 0, 1), rtol=1e-15)
    assert sol.ctx.kernel_name(3) == "odef::errors_partial_kernel<1, odef::TruthAnalytic<odef::ErrDecay>>"
    plain = pkg.solve(pkg.EnsembleProblem(pkg.ODEProblem("ErrDecayPlain", u0s[0], (0.0, 1.0), p), u0s=u0s), pkg.EK1(order=2),
                      pkg.EnsembleHIP(), dt=2.0 ** -5, adaptive=False)
    assert plain.errors is None and plain.u_analytic is None  # the reference returns `nothing`
    with pytest.raises(pkg.OdefError, match="has no `analytic` member and no reference is bound"):
        plain.ctx.solution_errors(0)
    with pytest.raises(pkg.OdefError, match="has no `analytic` member"):
        plain.ctx.field_bytes(h.errors_field(0, h.E_CHI2))


BOUND = [("lorenz63", 3, 130, 48, 2.0 ** -8, 1e-3), ("pleiades", 2, 5, 12, 2.0 ** -10, 1e-3)]


@pytest.mark.parametrize("name,q,N,ns,dt,scale", BOUND, ids=[c[0] for c in BOUND])
def test_bound_reference_from_a_finer_solve(pkg, name, q, N, ns, dt, scale):
    """`appxtrue` for a field without a closed form: a solve with a quarter of the step, its smoothed dense output on the coarse
    grid, rows 0..d-1 bound as ODEF_E_REFERENCE.  Lorenz-63 (d = 3, registers) and Pleiades (d = 28, LDS column)."""
    import torch

    h = _host()
    vf = orc.vector_field(name)
    grid = np.arange(ns + 1) * dt
    with pkg.Context(name, q, h.EK1_ID, N, smooth=True) as fine:
        fine.set_problem_perturbed(vf.u0, vf.p, 0.0, scale)
        fine.solve_fixed(np.arange(4 * ns + 1) * (dt / 4))
        fine.smooth()
        m, _ = fine.dense_output(grid, True)
    d = len(vf.u0)
    truth = np.ascontiguousarray(m[:, :d, :])
    buf = torch.from_numpy(truth).to("cuda")
    torch.cuda.synchronize()
    with pkg.Context(name, q, h.EK1_ID, N, smooth=True) as ctx:
        ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, scale)
        ctx.solve_fixed(grid)
        ctx.smooth()
        assert np.all(ctx.get(h.F_RETCODE) == 0)
        with pytest.raises(pkg.OdefError, match="has no `analytic` member and no reference is bound"):
            ctx.solution_errors(0)
        ctx.bind_reference(buf.data_ptr(), truth.nbytes - 8)
        with pytest.raises(pkg.OdefError, match="ODEF_E_REFERENCE buffer holds"):
            ctx.solution_errors(0)
        ctx.bind_reference(buf.data_ptr(), truth.nbytes)
        assert ctx.field_bytes(h.errors_field(0, h.E_L2)) == 8 * N
        assert ctx.field_bytes(h.errors_field(1, h.E_U_ANALYTIC)) == truth.nbytes
        for source in (0, 1):
            got, _ = _check(ctx, source, truth, False, f"{name} EK1({q}) bound reference, source {source}")
            assert np.all(got["nused"] == ns + 1) and np.all(np.isfinite(got["chi2"]))
        assert ctx.kernel_name(3) == f"odef::errors_partial_kernel<{d if d <= 8 else 0}, odef::TruthBuffer>"
        np.testing.assert_array_equal(ctx.get(h.errors_field(0, h.E_U_ANALYTIC)), truth)
        np.testing.assert_array_equal(buf.cpu().numpy(), truth)  # read only
        if name == "lorenz63":
            ctx.solve_adaptive(grid[-1], abstol=1e-6, reltol=1e-4, dt0=dt, max_steps=ns)
            with pytest.raises(pkg.OdefError, match="give the vector field an `analytic` member"):
                ctx.solution_errors(0)
        ctx.bind_reference(0, 0)
    del buf


def test_two_shards_equal_one_context(pkg):
    h = _host()
    vf = orc.vector_field("linear")
    N, grid = 131, np.arange(33) * 2.0 ** -5
    u0s = _u0s(N, 2, vf.u0, 3)
    with h.DeviceGroup("linear", 3, h.EK1_ID, N, 2, device_ids=[0, 0], smooth=True) as grp:
        assert grp.shard(0) == (0, 66) and grp.shard(1) == (66, 65)
        grp.set_problem(u0s, vf.p, 0.0)
        grp.solve_fixed(grid)
        grp.smooth()
        both = [grp.solution_errors(source) for source in (0, 1)]
    with pkg.Context("linear", 3, h.EK1_ID, N, smooth=True) as ctx:
        ctx.set_problem(u0s, vf.p, 0.0)
        ctx.solve_fixed(grid)
        ctx.smooth()
        for source in (0, 1):
            one = ctx.solution_errors(source)
            for k in one:
                assert both[source][k].shape == (N,)
                np.testing.assert_array_equal(both[source][k], one[k])


@pytest.mark.parametrize("q", [1, 2, 3, 4])
def test_convergence_orders_from_device_side_errors(pkg, q):
    """The reference's own convergence check (test/convergence.jl:9-28): u' = 1.01 u, u0 = 1/2 on (0, 1), EK0(order = q); the
    estimated order of `final` and `l2` over three step sizes -- DiffEqDevTools' mean of log2 ratios -- is q + 1 within its
    TESTTOL = 0.2 (+ 0.1 for l2 at q >= 4), from sol.errors computed on the device."""
    prob = pkg.ODEProblem("linear", np.array([0.5, 0.5]), (0.0, 1.0), np.array([1.01, 1.01]))
    dts = [2.0 ** -k for k in (5, 6, 7)]
    errs = {"final": [], "l2": [], "l∞": []}
    for dt in dts:
        sol = pkg.solve(prob, pkg.EK0(order=q), pkg.EnsembleHIP(), dt=dt, adaptive=False)
        e = sol.errors
        for k in errs:
            errs[k].append(float(e[k][0]))
    est = {k: float(np.mean(np.log2(np.array(v[:-1]) / np.array(v[1:])))) for k, v in errs.items()}
    print(f"EK0({q}): errors {errs}  estimated orders {est}")
    assert abs(est["final"] - (q + 1)) <= 0.2
    assert abs(est["l2"] - (q + 1)) <= (0.2 if q <= 3 else 0.3)
