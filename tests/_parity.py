"""Parity helpers shared by the CPU (emulated-lane) and GPU tests.

Tolerances.  The hard bar of BASELINE.json (posterior means of the solution within 1e-8
relative) is asserted at 1e-10 on E0*mu (`sol.u`).  Higher-derivative components of the
state and the covariances are *ill-conditioned in the reference's own arithmetic*: a 1-ulp
change of u0 moves the reference's u''' by up to 1e-8 relative on Lorenz-63.

Where an EXACT evaluation of the reference algorithm exists (tests/golden/exact_lorenz_mp.npz: mpmath, 50 digits,
1 024 steps, filter and smoother; exact_pleiades_ld.npz: x87 extended precision, 24 steps; generator
tests/golden/make_exact.py) the question asked is the right one -- is the device as close to the exact result as the
float64 oracle is: `check_against_exact` requires |device - exact| <= EXACT_FACTOR x |oracle - exact| per derivative
block and for the covariance.  Measured ratios (tests/test_emul_parity.py prints nothing, the numbers are in DESIGN.md
section 4): lane kernels 1.3-2.0, row-team kernels 0.4-9.7, tiled D = 168 kernel 0.9-12.  The other small-state shapes (D = 4 ... 18,
orders 1 ... 5, EK0, the fixed diffusion model) and Lorenz-96 on the matrix cores have extended-precision fixtures of their own
(make_exact.py --small) and `check_against_exact_floored`, the same bar with a floor of one rounding per step: measured 0.6-8.6.

fixedMAP, the MV diffusion models, IEKS and the time-dependent field `forced` have such fixtures too (make_exact.py --models,
tests/test_exact_models_emul.py, tests/test_gpu_exact_models.py).

Elsewhere (adaptive solves, run-time compiled fields) the tolerance is calibrated on the oracle itself: `noise` = spread of the oracle under 1-ulp input
perturbations, and two fp64 implementations are required to agree within NOISE_FACTOR x noise (+ a 1e-11 floor).
How the factor relates to the exact fixtures: on Lorenz-63 the oracle's 1-ulp spread is 2x its distance from the exact
result, so a device 12x as far from exact as the oracle is sits at most (12 + 1) / 2 = 6.5 noise units from the oracle.
The spread of six random 1-ulp perturbations is a noisy yardstick, though: the largest ratio the GPU suite meets where
no exact fixture exists is 240 (Pleiades EK0(3), top derivative block of the SMOOTHED state through the D = 168 team
smoother, which factorises differently from the oracle); NOISE_FACTOR = 512 covers that with a factor 2 (round 1: 1000,
with nothing behind it).
"""
import numpy as np

import odefilter_oracle as orc

NOISE_FACTOR = 512.0
EXACT_FACTOR = 16.0
U_RTOL = 1e-10
FLOOR = 1e-11


def block_err(a, b, d):
    """max abs error per derivative block, relative to the block's max magnitude over the run."""
    nb = a.shape[-1] // d
    out = []
    for j in range(nb):
        sl = slice(j * d, (j + 1) * d)
        out.append(np.nanmax(np.abs(a[..., sl] - b[..., sl])) / (np.nanmax(np.abs(b[..., sl])) + 1e-300))
    return np.array(out)


def cov_err(a, b):
    """per-step max-norm relative covariance error, maximised over steps."""
    scale = np.nanmax(np.abs(b), axis=(-2, -1), keepdims=True) + 1e-300
    return float(np.nanmax(np.abs(a - b) / scale))


_NOISE_CACHE = {}


def oracle_noise(vf, alg, u0, solve_kwargs, smoothed, n_pert=6):
    """Spread of the oracle under 1-ulp relative perturbations of u0 (max over `n_pert` random sign
    patterns): returns (base solution, mean-noise per derivative block, cov-noise).  Filter and
    smoothed statistics come from the same oracle runs (cached)."""
    key = (vf.name, alg.kind, alg.order, alg.diffusionmodel, tuple(np.asarray(u0).tolist()),
           tuple(sorted((k, str(v)) for k, v in solve_kwargs.items())), n_pert)
    if key not in _NOISE_CACHE:
        alg_s = orc.Alg(alg.kind, alg.order, alg.diffusionmodel, True)
        base = orc.solve(vf, alg_s, u0=u0, **solve_kwargs)
        rng = np.random.default_rng(7)
        noise = {False: [np.zeros(alg.order + 1), 0.0], True: [np.zeros(alg.order + 1), 0.0]}
        for _ in range(n_pert):
            du = u0 * (1.0 + (rng.integers(0, 2, size=u0.shape) * 2 - 1) * 2.0**-52)
            kw = {k: v for k, v in solve_kwargs.items() if k != "tgrid"}
            s = orc.solve(vf, alg_s, u0=du, tgrid=None if solve_kwargs.get("adaptive") else base.t, **kw)
            if len(s.t) != len(base.t):
                continue
            for sm in (False, True):
                noise[sm][0] = np.maximum(noise[sm][0], block_err(s.means(smoothed=sm), base.means(smoothed=sm), vf.d))
                noise[sm][1] = max(noise[sm][1], cov_err(s.covs(smoothed=sm), base.covs(smoothed=sm)))
        _NOISE_CACHE[key] = (base, noise)
    base, noise = _NOISE_CACHE[key]
    return base, noise[smoothed][0], noise[smoothed][1]


def check_against_oracle(mean, cov, ref_mean, ref_cov, d, noise_m, noise_c, what=""):
    be = block_err(mean, ref_mean, d)
    assert be[0] <= U_RTOL, f"{what}: posterior mean of the solution off by {be[0]:.2e} (> {U_RTOL})"
    tol = np.maximum(FLOOR, NOISE_FACTOR * noise_m)
    tol[0] = U_RTOL
    assert np.all(be <= tol), f"{what}: derivative-block mean errors {be} exceed calibrated tolerances {tol}"
    ce = cov_err(cov, ref_cov)
    ctol = max(1e-9, NOISE_FACTOR * noise_c)
    assert ce <= ctol, f"{what}: covariance error {ce:.2e} exceeds calibrated tolerance {ctol:.2e}"
    return be, ce


def check_against_exact(mean, cov, exact_mean, exact_cov, oracle_block_err, oracle_cov_err, d, what=""):
    """|device - exact| <= EXACT_FACTOR x |oracle - exact|, per derivative block (floor: 4 ulp of the block scale) and for
    the covariance; the solution block additionally at U_RTOL."""
    be = block_err(mean, exact_mean, d)
    assert be[0] <= U_RTOL, f"{what}: posterior mean of the solution off by {be[0]:.2e} from the exact result"
    tol = np.maximum(EXACT_FACTOR * np.asarray(oracle_block_err), 1e-15)
    assert np.all(be <= tol), f"{what}: block errors vs exact {be} exceed {EXACT_FACTOR} x the oracle's {oracle_block_err}"
    ce = cov_err(cov, exact_cov)
    assert ce <= EXACT_FACTOR * float(oracle_cov_err), f"{what}: covariance error vs exact {ce:.2e} exceeds {EXACT_FACTOR} x the oracle's {float(oracle_cov_err):.2e}"
    return be, ce


def check_against_exact_fixture(fx, k, mean_f, cov_f, mean_s, cov_s, d, what=""):
    """tests/golden/exact_pleiades_*_smooth_ld.npz (make_exact.py: filter and smoother in extended precision, trajectories
    fx["trajs"], covariances at ONE record each as packed lower triangles): trajectory number `k` of the fixture.  mean_* are
    [n_save, D], cov_* [n_save, D, D] of the device.  The yardstick per derivative block / covariance is the float64 oracle's
    own distance from the exact result, the LARGEST over the fixture's trajectories: where that arithmetic is rounding noise
    (order 5 at dt = 2^-10: the first residuals are h^5-small, the oracle's diffusions up to 300x off) a single trajectory's
    distance is a lottery ticket, not a scale."""
    D = mean_f.shape[-1]
    il = np.tril_indices(D)
    out = {}
    for name, mean, cov, rec in (("filt", mean_f, cov_f, int(fx["cov_record_filt"])), ("smooth", mean_s, cov_s, int(fx["cov_record_smooth"]))):
        exact_mean = fx["mean_" + name][k]
        be = block_err(mean, exact_mean, d)
        assert be[0] <= U_RTOL, f"{what} {name}: posterior mean of the solution off by {be[0]:.2e} from the exact result"
        tol = np.maximum(EXACT_FACTOR * fx["oracle_block_err_" + name].max(axis=0), 1e-15)
        assert np.all(be <= tol), f"{what} {name}: block errors vs exact {be} exceed {EXACT_FACTOR} x the oracle's {fx['oracle_block_err_' + name].max(axis=0)}"
        exact_cov = np.zeros((D, D))
        exact_cov[il] = fx[f"cov_{name}_tril"][k]
        exact_cov = exact_cov + np.tril(exact_cov, -1).T
        ce = cov_err(cov[rec][None], exact_cov[None])
        ctol = EXACT_FACTOR * float(fx["oracle_cov_err_" + name].max())
        assert ce <= ctol, f"{what} {name}: covariance of record {rec} off by {ce:.2e} from the exact one, {EXACT_FACTOR} x the oracle's distance is {ctol:.2e}"
        out[name] = (be, ce)
    return out


def check_against_exact_floored(fx, k, mean_f, cov_f, mean_s, cov_s, d, diffusions=None, loglik=None, what=""):
    """The fixtures of make_exact.py --small: tests/golden/exact_small_*_ld.npz (covariances of EVERY record, [traj, record,
    TRI]) and exact_lorenz96_*_smooth_ld.npz (the layout of the Pleiades fixtures, covariances at ONE record each): trajectory
    number `k` of the fixture.  Per derivative block and for the covariance, filter and smoothed,

        |device - exact| <= EXACT_FACTOR x max(largest oracle distance over the fixture's trajectories, n_steps 2^-52)

    The floor is one rounding per step: at order 1 the oracle itself is a few ulps from the exact result (4e-15), and a
    kernel that rounds in another order is not 16 x worse for being 20 ulps away after 64 steps.  The solution block is held to
    U_RTOL as well.  diffusions [n_steps] (the MV diffusion models: [n_steps, d], every entry relative to its own exact value) and
    loglik, when given, are held to the same form relative to their magnitude (the fixture's oracle_diffusion_err /
    oracle_loglik_err).  Returns the ratios error / yardstick: {"filt": (per block, cov),
    "smooth": (per block, cov), "diffusion": r, "loglik": r}."""
    D = mean_f.shape[-1]
    il = np.tril_indices(D)
    floor = int(fx["nsteps"]) * 2.0**-52
    one_record = "cov_record_filt" in fx.files
    out = {}
    for name, mean, cov in (("filt", mean_f, cov_f), ("smooth", mean_s, cov_s)):
        be = block_err(mean, fx["mean_" + name][k], d)
        assert be[0] <= U_RTOL, f"{what} {name}: posterior mean of the solution off by {be[0]:.2e} from the exact result"
        yard = np.maximum(fx["oracle_block_err_" + name].max(axis=0), floor)
        assert np.all(be <= EXACT_FACTOR * yard), f"{what} {name}: block errors vs exact {be} exceed {EXACT_FACTOR} x {yard} (the oracle's distance, floored at {floor:.1e})"
        tril = fx[f"cov_{name}_tril"][k]
        exact_cov = np.zeros(tril.shape[:-1] + (D, D))
        exact_cov[..., il[0], il[1]] = tril
        exact_cov = exact_cov + np.swapaxes(np.tril(exact_cov, -1), -1, -2)
        if one_record:
            rec = int(fx["cov_record_" + name])
            ce = cov_err(cov[rec][None], exact_cov[None])
        else:
            ce = cov_err(cov, exact_cov)
        cyard = max(float(fx["oracle_cov_err_" + name].max()), floor)
        assert ce <= EXACT_FACTOR * cyard, f"{what} {name}: covariance off by {ce:.2e} from the exact one, {EXACT_FACTOR} x the oracle's distance (floored) is {EXACT_FACTOR * cyard:.2e}"
        out[name] = (be / yard, ce / cyard)
    if diffusions is not None:
        ex = fx["diffusions"][k]
        assert np.shape(diffusions) == ex.shape, f"{what}: diffusions of shape {np.shape(diffusions)}, the fixture's are {ex.shape}"
        de = float(np.max(np.abs(np.asarray(diffusions) - ex) / np.abs(ex)))
        dyard = max(float(np.max(fx["oracle_diffusion_err"])), floor)
        assert de <= EXACT_FACTOR * dyard, f"{what}: diffusions off by {de:.2e} relative from the exact ones, {EXACT_FACTOR} x the oracle's distance (floored) is {EXACT_FACTOR * dyard:.2e}"
        out["diffusion"] = de / dyard
    if loglik is not None:
        ex = float(fx["loglik"][k])
        le = abs(float(loglik) - ex) / abs(ex)
        lyard = max(float(np.max(fx["oracle_loglik_err"])), floor)
        assert le <= EXACT_FACTOR * lyard, f"{what}: log-likelihood off by {le:.2e} relative from the exact one, {EXACT_FACTOR} x the oracle's distance (floored) is {EXACT_FACTOR * lyard:.2e}"
        out["loglik"] = le / lyard
    return out


def check_initial_record_floored(fx, k, mean_f, d, what):
    """Record 0 on its own: blocks 1 ... q of the Taylor-mode initialisation, which for f(u, p, t) carry the time jet [t0, 1, 0, ...].
    The bar of the blocks over the run, relative to the record's own block magnitudes: the recursion is a few dozen operations,
    so the floor of one rounding per step of the run is a generous yardstick for it."""
    floor = int(fx["nsteps"]) * 2.0**-52
    be = block_err(mean_f[:1], fx["mean_filt"][k][:1], d)
    yard = np.maximum(fx["oracle_block_err_filt"].max(axis=0), floor)
    assert np.all(be <= EXACT_FACTOR * yard), f"{what}: blocks of the initial record off by {be} from the exact ones, bar {EXACT_FACTOR} x {yard}"
    return be / yard
