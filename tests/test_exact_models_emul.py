"""The device source of fixedMAP, the MV diffusion models, IEKS and the time-dependent field `forced`, compiled for the host
(tests/emul), against EXTENDED-PRECISION evaluations of the reference algorithm (tests/golden/exact_model_*_ld.npz, generator
`make_exact.py --models`, cases `_exact_cases.MODEL_CASES`): each is as close to the exact result as the float64 reference is
(factor 16, `_parity.check_against_exact_floored`), block by block -- the derivative blocks and the initial record included --,
for the covariances of every record, the diffusions (MV: every component) and the log-likelihood, on all four fixture
trajectories.  Until these fixtures the four families were held to 512 x the oracle's 1-ulp spread or to fixed rtols of 1e-6 ...
1e-3 on the covariances, several hundred times the oracle's distance from the exact result.

The pre-flight of tests/test_gpu_exact_models.py, which runs the same cases through the C ABI on the real kernels."""
import ctypes as C

import numpy as np
import pytest

import _emul as E
import _exact_cases as X
import _parity as P
import test_ieks_emul as TI
import test_time_emul as TT

orc = E.orc
NT = X.SMALL_NTRAJ
# emulated kernels: the numbering of emul_ieks.cpp / emul_time.cpp
KERNELS = {"lane": 0, "lane_lag": 1, "rows": 2}


def check_fixture(case, fx, r, kernels):
    """r: mean, cov, smean, scov [traj, record, ...], diff [traj, record] or [traj, record, d] (record 0 unused), loglik [traj]."""
    family, rhs, kind, q, diffusion, dt = case
    d = X.MODEL_DIM[rhs]
    with_loglik = diffusion in ("dynamic", "dynamicMV")
    ratios = []
    for k in range(NT):
        ratios.append(P.check_against_exact_floored(fx, k, r["mean"][k], r["cov"][k], r["smean"][k], r["scov"][k], d, diffusions=r["diff"][k][1:],
                                                    loglik=r["loglik"][k] if with_loglik else None,
                                                    what=f"emulation {X.model_id(case)} {kernels} traj {k}"))
    if not with_loglik:
        assert np.isnan(r["loglik"]).all()  # src/integrator_utils.jl:6
    return ratios


def run_map(case, kernels):
    """emul_solve with the on-line MAP update (fixed_diffusion = 2) and the postamble.  "lane": lane filter, then the lane
    smoother (D <= 12) or the LDS row teams; "rows": the row-team filter and the DPP row-team smoother (D <= 16)."""
    family, rhs, kind, q, diffusion, dt = case
    fx = X.load(X.model_name(case))
    vf = orc.vector_field(rhs)
    r = E.emul_solve(vf.rhs_id, vf.d, q, kind == "EK1", fx["u0s"], vf.p, tgrid=fx["t"], everystep={"lane": True, "rows": 3}[kernels],
                     smooth=True, fixed_diffusion=2, rescale_static=True)
    assert (r["retcode"] == 0).all() and (r["naccept"] == X.SMALL_NSTEPS).all()
    return check_fixture(case, fx, r, kernels)


def run_mv(case, kernels):
    """tests/emul/emul_mv.cpp: filter_fixed_lane<..., MV = true> ("lane_lag": with lagged record stores), the postamble of :fixedMV,
    the MV instantiation of the row-team smoother."""
    family, rhs, kind, q, diffusion, dt = case
    fx = X.load(X.model_name(case))
    vf = orc.vector_field(rhs)
    r = E.emul_solve_mv(vf.rhs_id, vf.d, q, fx["u0s"], vf.p, fx["t"], diffusion, lag=kernels == "lane_lag")
    assert (r["retcode"] == 0).all() and (r["naccept"] == X.SMALL_NSTEPS).all()
    assert r["diff"].shape == (NT, X.SMALL_NSTEPS + 1, vf.d)
    return check_fixture(case, fx, r, kernels)


def run_forced(case, kernels):
    """tests/emul/emul_time.cpp around RhsForced: P.t0 in the Taylor-mode initialisation, P.tgrid[n + 1] in every step."""
    family, rhs, kind, q, diffusion, dt = case
    fx = X.load(X.model_name(case))
    vf = X.model_field(case)
    r = TT.emul_time(q, kind == "EK1", fx["u0s"], vf.p, diffusion, KERNELS[kernels], grid=fx["t"])
    assert (r["retcode"] == 0).all()
    r = dict(r, diff=r["diff"][:, :, 0])
    for k in range(NT):
        P.check_initial_record_floored(fx, k, r["mean"][k], 2, f"emulation {X.model_id(case)} {kernels} traj {k}")
    return check_fixture(case, fx, r, kernels)


def run_ieks(case, kernels):
    """solve_ieks on the emulated kernels, chained as tests/test_ieks_emul.py chains them: iteration 1 on the EK1 kernels, iterations
    2 and 3 on the IEKS kernels with the emulated smoother's u of the previous one as linearisation points; the third iteration
    against the fixture."""
    family, rhs, kind, q, diffusion, dt = case
    fx = X.load(X.model_name(case))
    assert int(fx["iterations"]) == X.IEKS_ITERATIONS
    vf = orc.vector_field(rhs)
    d, D = vf.d, vf.d * (q + 1)
    TRI = D * (D + 1) // 2
    kernel = KERNELS[kernels]
    L = TI.lib()
    u0_dev = np.ascontiguousarray(fx["u0s"].T)
    p = np.ascontiguousarray(vf.p)
    At, Qt, QLt = E.prior_tables(q)
    tg = np.ascontiguousarray(fx["t"])
    hs = np.ascontiguousarray(np.diff(tg))
    n_save = len(tg)
    uniq, inv = np.unique(hs, return_inverse=True)
    ptab = np.zeros((len(uniq), L.emul_tab_stride()))
    for k, h in enumerate(uniq):
        L.emul_precond_fill(q, float(h), float(h) ** (-q - 1 / 2), E._p(ptab[k]))
    tab_idx = np.ascontiguousarray(inv.astype(np.int32))
    ctrl = np.zeros(10)
    a = E.EmulArgs()
    a.rhs, a.q, a.ek1, a.adaptive = vf.rhs_id, q, 1, 0
    a.N, a.u0, a.p, a.p_shared = NT, E._p(u0_dev), E._p(p), 1
    a.At, a.Qt, a.QLt = E._p(At), E._p(Qt), E._p(QLt)
    a.hs, a.ptab, a.tab_idx, a.nsteps = E._p(hs), E._p(ptab), E._p(tab_idx, E.ip), len(hs)
    a.t0, a.ctrl, a.max_save = float(tg[0]), E._p(ctrl), 0
    a.everystep, a.fixed_diffusion, a.want_loglik = 1, {"dynamic": 0, "fixed": 1, "fixedMAP": 2}[diffusion], 1
    lin = None
    for _ in range(X.IEKS_ITERATIONS):
        mean = np.zeros((n_save, D, NT)); cov = np.zeros((n_save, TRI, NT)); diff = np.zeros((n_save, NT))
        tsave = np.zeros((n_save, NT)); loglik = np.zeros(NT)
        ints = [np.zeros(NT, np.int32) for _ in range(6)]
        a.mean, a.cov, a.diff, a.tsave, a.loglik = E._p(mean), E._p(cov), E._p(diff), E._p(tsave), E._p(loglik)
        a.naccept, a.nreject, a.nf, a.njac, a.nsaved, a.retcode = [E._p(x, E.ip) for x in ints]
        if lin is None:  # the empty field: the EK1 kernels
            a.everystep = {0: 1, 1: 2, 2: 3}[kernel]
            assert L.emul_filter(C.byref(a)) == 0
        else:
            a.everystep = 1
            assert L.emul_filter_ieks(C.byref(a), E._p(lin), kernel) == 0
        assert (ints[5] == 0).all()
        if diffusion != "dynamic":  # postamble! (src/integrator_utils.jl:4-18), the device's scale_cov_kernel
            cov *= diff[-1][None, None, :]
            diff[1:] = diff[-1][None, :]
            loglik[:] = np.nan
        smean = np.zeros_like(mean); scov = np.zeros_like(cov)
        a.smean, a.scov, a.n_save = E._p(smean), E._p(scov), n_save
        a.everystep = 3 if kernel == 2 else 1  # the DPP row-team smoother behind the row-team filter
        assert L.emul_smooth(C.byref(a), d) == 0
        lin = np.ascontiguousarray(smean[:, :d, :])  # odef_smooth: rows 0..d-1 of every SMOOTH_MEAN save
    r = dict(mean=mean.transpose(2, 0, 1), cov=E.unpack_tril(cov.transpose(2, 0, 1), D), smean=smean.transpose(2, 0, 1),
             scov=E.unpack_tril(scov.transpose(2, 0, 1), D), diff=diff.T, loglik=loglik)
    return check_fixture(case, fx, r, kernels)


RUNNERS = {"map": run_map, "mv": run_mv, "forced": run_forced, "ieks": run_ieks}


def emul_kernels(case):
    """The emulated kernel sets of a case: the row-team kernels serve state dimension <= 16, the MV models are the lane filter's."""
    D = X.MODEL_DIM[case[1]] * (case[3] + 1)
    if case[0] == "map":
        return ["lane"] + (["rows"] if D <= 16 else [])
    if case[0] == "mv":
        return ["lane", "lane_lag"]
    return ["lane", "lane_lag"] + (["rows"] if D <= 16 else [])


def check_emulation(case, kernels):
    return RUNNERS[case[0]](case, kernels)


def _params(family):
    return [pytest.param(c, k, id=f"{X.model_id(c)}-{k}") for c in X.model_cases(family) for k in emul_kernels(c)]


@pytest.mark.parametrize("case,kernels", _params("map"))
def test_fixed_map_against_extended_precision(case, kernels):
    """The on-line MAP update of the global diffusion on the lane and row-team kernels."""
    check_emulation(case, kernels)


@pytest.mark.parametrize("case,kernels", _params("mv"))
def test_mv_models_against_extended_precision(case, kernels):
    """:dynamicMV / :fixedMV: the MV lane filter with and without lagged stores, the MV row-team smoother; d diffusions per step."""
    check_emulation(case, kernels)


@pytest.mark.parametrize("case,kernels", _params("ieks"))
def test_ieks_third_iteration_against_extended_precision(case, kernels):
    """Three chained iterations on the IEKS lane (plain, lagged stores) and row-team kernels, one case per diffusion model."""
    check_emulation(case, kernels)


@pytest.mark.parametrize("case,kernels", _params("forced"))
def test_forced_field_against_extended_precision(case, kernels):
    """f(u, p, t): every derivative block of every record, record 0 -- the Taylor-mode initialisation with its time jet -- included."""
    check_emulation(case, kernels)


def test_the_families_are_covered():
    """What the fixtures are for: every model the four families add, the widest MV instantiation that can be admitted, one IEKS
    case per diffusion model IEKS takes with one at D = 12, EK0 and EK1 of `forced` with orders 1 ... 3."""
    dim = lambda c: X.MODEL_DIM[c[1]] * (c[3] + 1)  # noqa: E731
    assert {c[4] for c in X.model_cases("map")} == {"fixedMAP"} and len(X.model_cases("map")) == 3
    assert {c[4] for c in X.model_cases("mv")} == {"dynamicMV", "fixedMV"} and {c[2] for c in X.model_cases("mv")} == {"EK0"}
    assert max(dim(c) for c in X.model_cases("mv") if c[4] == "dynamicMV") >= 10
    assert max(c[3] for c in X.model_cases("mv") if c[4] == "dynamicMV") >= 4
    assert {c[4] for c in X.model_cases("ieks")} == {"dynamic", "fixed", "fixedMAP"} and 12 in {dim(c) for c in X.model_cases("ieks")}
    assert {(c[2], c[3]) for c in X.model_cases("forced")} >= {("EK0", 2), ("EK1", 3)} and {c[3] for c in X.model_cases("forced")} == {1, 2, 3}
    assert len({X.model_name(c) for c in X.MODEL_CASES}) == len(X.MODEL_CASES)


def test_model_fixtures_meet_their_admission_condition():
    """The generator asserts it before writing; a fixture edited or regenerated by other means is caught here: the reference's
    diffusions within 1e-4 relative of the extended-precision ones on every fixture trajectory (MV: every component; the
    rounding-noise regimes, e.g. Lotka-Volterra EK0(5) dynamicMV at 2^-6, sit at 5e-3 and above), time grid and initial values as
    documented, MV diffusions stored as [traj, step, d]."""
    for case in X.MODEL_CASES:
        family, rhs, kind, q, diffusion, dt = case
        fx = X.load(X.model_name(case))
        d = X.MODEL_DIM[rhs]
        assert float(np.max(fx["oracle_diffusion_err"])) <= 1e-4, X.model_id(case)
        assert fx["oracle_diffusion_err"].shape == (NT,)
        np.testing.assert_array_equal(fx["u0s"], orc.ensemble_u0(X.model_field(case).u0, NT, 1e-2))
        np.testing.assert_array_equal(fx["t"], X.model_grid(case))
        assert int(fx["nsteps"]) == X.SMALL_NSTEPS and int(fx["order"]) == q and str(fx["diffusionmodel"]) == diffusion
        assert str(fx["family"]) == family and str(fx["kind"]) == kind and float(fx["dt"]) == dt
        D = d * (q + 1)
        assert fx["mean_filt"].shape == fx["mean_smooth"].shape == (NT, X.SMALL_NSTEPS + 1, D)
        assert fx["cov_filt_tril"].shape == fx["cov_smooth_tril"].shape == (NT, X.SMALL_NSTEPS + 1, D * (D + 1) // 2)
        assert fx["diffusions"].shape == ((NT, X.SMALL_NSTEPS, d) if family == "mv" else (NT, X.SMALL_NSTEPS))
        assert np.isfinite(fx["loglik"]).all() == (diffusion in ("dynamic", "dynamicMV"))
        if diffusion in ("fixed", "fixedMAP", "fixedMV"):  # the postamble: one diffusion for the whole solve
            assert (fx["diffusions"] == fx["diffusions"][:, :1]).all()
