"""The HIP kernels (through the C ABI) against EXTENDED-PRECISION evaluations of the reference algorithm, for every small-state
instantiation other than Lorenz-63 EK1(3) and for Lorenz-96 on the matrix-core kernels (tests/golden/exact_small_*_ld.npz,
exact_lorenz96_*_smooth_ld.npz; generator `make_exact.py --small`).  The question is the one test_pleiades_ensemble_parity asks
at D = 84 ... 168: is the device as close to the exact result of the reference algorithm as the float64 oracle is (factor 16,
`_parity.check_against_exact_floored`) -- per derivative block, for the covariances, the diffusions and the log-likelihood.  The
same cases pass in emulation first (tests/test_exact_emul.py).  Needs a real MI355X: run with `-m gpu`."""
import numpy as np
import pytest

import _exact_cases as X
import _parity as P
import odefilter_oracle as orc

pytestmark = pytest.mark.gpu

N = 70  # ragged for 64-lane wavefronts (lane kernels) and for the four-trajectory waves of the row-team kernels
CHECKED = (0, 1, 2, 3, 66, 67, 68, 69)  # the first wavefront / team wave and the ragged last ones

COMBOS = [(case, f, s) for case in X.SMALL_CASES for f in X.filter_families(X.SMALL_DIM[case[0]] * (case[2] + 1))
          for s in X.smoother_families(X.SMALL_DIM[case[0]] * (case[2] + 1))]


def _alg(pkg, kind, order, diffusion="dynamic"):
    return (pkg.EK1 if kind == "EK1" else pkg.EK0)(order=order, diffusionmodel=diffusion, smooth=True)


def solve_small(pkg, case, filt, smoother, setenv):
    """The fixture's four trajectories, k at every index i with i % 4 == k, on the fixture's save times, with the launch-time
    overrides that force the given filter and smoother family.  Returns (fixture, solution)."""
    rhs, kind, q, diffusion, dt = case
    fx = X.load(X.small_name(rhs, kind, q, diffusion))
    vf = orc.vector_field(rhs)
    for k, v in {**X.FILTER_ENV[filt], **X.SMOOTH_ENV[smoother]}.items():
        setenv(k, v)
    u0s = fx["u0s"][np.arange(N) % X.SMALL_NTRAJ]
    prob = pkg.EnsembleProblem(pkg.ODEProblem(rhs, u0s[0], (0.0, float(fx["t"][-1])), vf.p), u0s=u0s)
    sol = pkg.solve(prob, _alg(pkg, kind, q, diffusion), pkg.EnsembleHIP(), tstops=fx["t"], adaptive=False)
    return fx, sol


def check_small(fx, sol, case, filt, smoother):
    rhs, kind, q, diffusion, dt = case
    d = X.SMALL_DIM[rhs]
    assert sol.retcode == ["Success"] * N
    np.testing.assert_array_equal(sol.t, fx["t"])
    # the forced families ran
    assert sol.ctx.kernel_name(0).startswith(X.filter_kernel_name(filt, rhs, q, kind == "EK1")), sol.ctx.kernel_name(0)
    assert sol.ctx.kernel_name(1) == X.smoother_kernel_name(smoother, d, q), sol.ctx.kernel_name(1)
    mf, cf, ms, cs = sol.x_filt_mean(), sol.x_filt_cov(), sol.x_smooth_mean(), sol.x_smooth_cov()
    diff, ll = sol.diffusions, sol.log_likelihood
    ratios = []
    for i in CHECKED:
        k = i % X.SMALL_NTRAJ
        ratios.append(P.check_against_exact_floored(fx, k, mf[i], cf[i], ms[i], cs[i], d, diffusions=diff[i],
                                                    loglik=None if diffusion == "fixed" else ll[i],
                                                    what=f"{X.case_id(case)} {filt}+{smoother} traj {i}"))
    if diffusion == "fixed":
        assert np.isnan(ll).all()  # src/integrator_utils.jl:6
    # copies of the same input are bit-identical wherever they sit: in a full wavefront or the ragged one, whichever lane or team
    first = np.arange(N) % X.SMALL_NTRAJ
    for name, a in (("filter mean", mf), ("filter cov", cf), ("smoothed mean", ms), ("smoothed cov", cs), ("diffusions", diff), ("loglik", ll)):
        np.testing.assert_array_equal(a, a[first], err_msg=f"{name}: copies of one trajectory differ by position")
    # sol.pu[1]: mean u0, zero covariance
    np.testing.assert_array_equal(mf[:, 0, :d], fx["u0s"][first])
    assert np.all(cf[:, 0] == 0.0)
    return ratios


@pytest.mark.parametrize("case,filt,smoother", COMBOS, ids=[f"{X.case_id(c)}-{f}+{s}" for c, f, s in COMBOS])
def test_small_state_kernels_against_extended_precision(pkg, case, filt, smoother, monkeypatch):
    """Every kernel family the launchers can select for the case's state dimension: {lane, row-team} filter x {lane, LDS
    row-team, DPP row-team} smoother for D <= 12, the row-team smoothers for D = 15, lane filter and LDS row teams for D = 18."""
    fx, sol = solve_small(pkg, case, filt, smoother, monkeypatch.setenv)
    check_small(fx, sol, case, filt, smoother)


def test_every_selectable_family_is_in_the_list():
    """csrc/ek_kernels.h LaunchFilterT / LaunchSmoothT: 2 x 3 families up to D = 12, 2 x 2 up to 16, 1 x 1 above."""
    n = {D: len(X.filter_families(D)) * len(X.smoother_families(D)) for D in (4, 12, 15, 16, 18)}
    assert n == {4: 6, 12: 6, 15: 4, 16: 4, 18: 1}
    assert len(COMBOS) == 11 * 6 + 4 + 1


def solve_lorenz96(pkg, kind, q, smoother, setenv):
    setenv("ODEF_SMOOTH_SPLIT", "1" if smoother == "split" else "0")
    fx = X.load(X.lorenz96_name(kind, q))
    vf = orc.vector_field("lorenz96")
    ns, dt = int(fx["nsteps"]), float(fx["dt"])
    ens = pkg.EnsembleProblem(pkg.ODEProblem("lorenz96", vf.u0, (0.0, ns * dt), vf.p), perturb_scale=1e-2)
    sol = pkg.solve(ens, _alg(pkg, kind, q), pkg.EnsembleHIP(), trajectories=6, dt=dt, adaptive=False)
    return fx, sol


def check_lorenz96(fx, sol, kind, q, smoother):
    assert sol.retcode == ["Success"] * 6
    assert "ek_filter_mfma_kernel<odef::RhsLorenz96" in sol.ctx.kernel_name(0)
    assert ("rts_smooth_sweeps_kernel<16" if smoother == "split" else "rts_smooth_mfma_kernel<16") in sol.ctx.kernel_name(1)
    u0s = sol.ctx.get(13).T
    mf, cf, ms, cs = sol.x_filt_mean(), sol.x_filt_cov(), sol.x_smooth_mean(), sol.x_smooth_cov()
    ratios = []
    for k, i in enumerate(fx["trajs"]):
        np.testing.assert_array_equal(u0s[i], fx["u0s"][k])
        ratios.append(P.check_against_exact_floored(fx, k, mf[i], cf[i], ms[i], cs[i], 16, diffusions=sol.diffusions[i],
                                                    loglik=sol.log_likelihood[i], what=f"lorenz96 {kind}({q}) {smoother} traj {i}"))
    return ratios


@pytest.mark.parametrize("smoother", ["split", "persistent"])
@pytest.mark.parametrize("kind,q", X.LORENZ96_CASES, ids=[f"{k}{q}" for k, q in X.LORENZ96_CASES])
def test_lorenz96_matrix_core_kernels_against_extended_precision(pkg, kind, q, smoother, monkeypatch):
    """filter_mfma.h / smooth_mfma.h on their second shape (d = 16, state dimension 48, 64, 96; Joseph form on the matrix cores
    against the oracle's square-root form), split and persistent smoother: trajectories 0 and 5 of the six, 12 steps."""
    fx, sol = solve_lorenz96(pkg, kind, q, smoother, monkeypatch.setenv)
    check_lorenz96(fx, sol, kind, q, smoother)
