"""The definition of the data log-likelihood at arbitrary times (tests/_datalik_times_reference.py) against what it must be
consistent with, on the CPU: the oracle's smoothed dense output for a single observation, the save-path reference for times on the
grid, its own float64 evaluation (the calibration of the tolerance), and an inference case on adaptive solves."""
import math

import numpy as np
import pytest

import _datalik_reference as dr
import _datalik_times_reference as tr
from _datalik_reference import orc


def _records_of(sol):
    """Device-layout filter records of one oracle solution: mean [n, D, 1], cov_tril [n, TRI, 1], diffusion [n, 1], t [n]."""
    D = sol.d * (sol.q + 1)
    il = np.tril_indices(D)
    mean = sol.means(False)[:, :, None]
    cov = sol.covs(False)[:, il[0], il[1]][:, :, None]
    diff = np.array([0.0] + list(sol.diffusions))[:, None]
    return np.ascontiguousarray(mean), np.ascontiguousarray(cov), diff, np.asarray(sol.t)


def _gauss_logpdf(y, m, S):
    v = y - m
    return -0.5 * (v @ np.linalg.solve(S, v) + np.linalg.slogdet(S)[1] + len(y) * math.log(2 * math.pi))


SOLVES = {
    "lv-ek1q3-adaptive": lambda: orc.solve(orc.vector_field("lotka_volterra"), orc.EK1(order=3), tspan=(0.0, 2.0), adaptive=True, dt=2.0 ** -6),
    "lv-ek1q3-fixed": lambda: orc.solve(orc.vector_field("lotka_volterra"), orc.EK1(order=3), tgrid=np.arange(33) * 2.0 ** -4),
    "lorenz-ek1q3-adaptive": lambda: orc.solve(orc.vector_field("lorenz63"), orc.EK1(order=3), tspan=(0.0, 0.25), adaptive=True, dt=2.0 ** -7),
    "lorenz-ek1q5-fixed": lambda: orc.solve(orc.vector_field("lorenz63"), orc.EK1(order=5), tgrid=np.arange(9) * 2.0 ** -5),
    "fhn-ek0q5-adaptive": lambda: orc.solve(orc.vector_field("fhn"), orc.EK0(order=5), tspan=(0.0, 1.0), adaptive=True, dt=2.0 ** -5),
    "lin1-ek0q1-fixed": lambda: orc.solve(dr._linear_field(1), orc.EK0(order=1), tgrid=np.arange(9) * 0.125),
}


@pytest.mark.parametrize("name", sorted(SOLVES))
def test_single_observation_equals_the_smoothed_dense_output(name):
    """M = 1: the sweep carries xi from the last record down to the node at tau, which is the smoothed posterior there, so the
    log-likelihood is the Gaussian log-density of y under oracle.dense_output(tau, smoothed=True) plus R."""
    sol = SOLVES[name]()
    consts = orc.make_consts(sol.d, sol.q)
    mean, cov, diff, t = _records_of(sol)
    comps = list(range(sol.d))
    r = np.full(sol.d, 1e-3)
    rng = np.random.default_rng(3)
    worst = 0.0
    for k in (0, 1, len(t) // 2, len(t) - 2):
        for f in (0.25, 0.8):
            tau = t[k] + f * (t[k + 1] - t[k])
            g = orc.dense_output(sol, consts, tau, smoothed=True)
            y = g.mu[: sol.d] + 0.03 * rng.standard_normal(sol.d)
            want = _gauss_logpdf(y, g.mu[: sol.d], g.cov()[: sol.d, : sol.d] + np.diag(r))
            got = tr.evaluate(mean, cov, diff, t, sol.d, sol.q, [tau], comps, y[None, :], r)
            rel = abs(float(got["loglik"][0]) - want) / abs(want)
            worst = max(worst, rel)
            assert rel <= 1e-10, (name, k, f, rel)
    print(f"{name}: worst relative difference to the dense output {worst:.3g}")


def test_times_on_the_grid_equal_the_save_path_reference_exactly():
    for name in ("lorenz-ek1q3-N130-c02-4th", "fhn-ek1q1-N65-repeat", "lin1-ek1q4-N65-save0"):
        c = dr.cases()[name]
        # (of a repeated time the chain observes the last copy; the save-path case names its copies, so take times of unique saves)
        t = np.asarray(c["t"])
        keep = [j for j, s in enumerate(c["saves"]) if (s + 1 >= len(t) or t[s + 1] != t[s]) and (s == 0 or t[s - 1] != t[s])]
        saves = [c["saves"][j] for j in keep]
        y = c["y"][..., keep, :]
        a = dr.evaluate(c["mean"], c["cov"], c["diff"], c["t"], c["d"], c["q"], saves, c["comps"], y, c["r"])
        b = tr.evaluate(c["mean"], c["cov"], c["diff"], c["t"], c["d"], c["q"], t[saves], c["comps"], y, c["r"])
        for k in tr.KEYS:
            assert np.array_equal(a[k], b[k]), (name, k)


def test_float64_numpy_evaluation_calibrates_the_tolerance():
    """The numpy float64 evaluation of the definition, prediction of the nodes included, against the longdouble reference on every
    input of the emulation tests and on oracle solves of the problems of the GPU tests, in units of `unit_bound`.  (The GPU tests'
    run-time compiled d = 4 field has no oracle twin; the pair (4, 2) is measured on the linear field.)"""
    worst = 0.0
    inputs = dict(tr.cases())
    inputs.update({"gpu:" + n: tr.gpu_like_case(n) for n in tr.GPU_PROBLEMS})
    for name, c in inputs.items():
        ref, f64 = tr.run_reference(c), tr.run_reference(c, np.float64)
        r = dr.ratios(f64, ref, tr.case_bound(c))
        print(name, {k: f"{v:.3g}" for k, v in r.items()})
        worst = max(worst, *r.values())
    print(f"numpy float64 / unit bound, worst: {worst:.3g} (C_MEASURED = {tr.C_MEASURED}, C_NUMPY = {tr.C_NUMPY})")
    assert worst <= tr.C_NUMPY
    assert tr.C_MEASURED / 4 <= worst <= tr.C_MEASURED  # the constant is the measured value rounded up
    assert tr.C_NUMPY == max(dr.C_NUMPY, tr.C_MEASURED) and tr.DEVICE_FACTOR == 16.0


def test_a_trajectory_whose_records_end_early_gives_nan():
    c = tr.cases()["lorenz-ek1q3-N65-ragged-short"]
    ref = tr.run_reference(c)
    assert list(np.flatnonzero(np.isnan(ref["loglik"].astype(float)))) == list(range(1, 65, 5))
    with pytest.raises(ValueError, match="before t0"):
        tr.evaluate(c["mean"], c["cov"], c["diff"], c["t"], c["d"], c["q"], [-0.1, 0.1], c["comps"], c["y"][:2], c["r"], c["nsaved"])


def inference_inputs(n_cand=33, M=16, sigma=1e-2):
    """Lotka-Volterra: candidates of p[0] around the truth 1.5; data from a tight solve plus seeded noise at 16 off-grid times."""
    vf = orc.vector_field("lotka_volterra")
    tight = orc.solve(vf, orc.EK1(order=5, smooth=True), tspan=(0.0, 2.0), adaptive=True, abstol=1e-10, reltol=1e-9, dt=2.0 ** -8)
    consts = orc.make_consts(vf.d, 5)
    times = 0.11 + (1.93 - 0.11) * np.linspace(0.0, 1.0, M) ** 1.05
    truth = np.array([orc.dense_output(tight, consts, float(s), smoothed=True).mu[: vf.d] for s in times])
    data = truth + sigma * np.random.default_rng(2022).standard_normal(truth.shape)
    ps = np.tile(vf.p, (n_cand, 1))
    ps[:, 0] = np.linspace(1.2, 1.8, n_cand)
    return vf, ps, times, data, sigma


def test_inference_on_adaptive_solves_picks_the_parameter_that_generated_the_data():
    vf, ps, times, data, sigma = inference_inputs()
    n = len(ps)
    u0s = np.tile(vf.u0, (n, 1))
    mean, cov, diff, T, ns = tr.adaptive_records(vf, orc.EK1(order=3, smooth=False), u0s, (0.0, 2.0), ps=ps, dt=2.0 ** -6)
    ll = tr.evaluate(mean, cov, diff, T, vf.d, 3, times, [0, 1], data, np.full(2, sigma ** 2), ns, dtype=np.float64)["loglik"]
    best = int(np.argmax(ll))
    print(f"argmax {best} of {n} (truth at {(n - 1) // 2}); loglik {ll[best]:.4g}, at the ends {ll[0]:.3g} {ll[-1]:.3g}")
    assert abs(best - (n - 1) // 2) <= 1
