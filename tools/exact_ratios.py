#!/usr/bin/env python3
"""Without arguments: how far the D = 84 / 112 / 168 kernels are from the extended-precision evaluation of the reference algorithm, in units of the
float64 oracle's own distance (tests/golden/exact_pleiades_*_smooth_ld.npz, generator tests/golden/make_exact.py): one JSON line
per fixture and kernel combination -- the numbers behind the factor-16 bar of tests/_parity.py check_against_exact_fixture.

--small: the same for the small-state kernels and for Lorenz-96 on the matrix-core kernels (tests/golden/exact_small_*_ld.npz,
exact_lorenz96_*_smooth_ld.npz): every kernel family the launchers can select, through the C ABI as tests/test_gpu_exact.py runs
them; ratios are error / max(oracle's distance, n_steps 2^-52), the largest over the checked trajectories
(check_against_exact_floored).  --small-emul: the host build of the device source instead (tests/test_exact_emul.py; no GPU).
--models / --models-emul: the same for fixedMAP, the MV diffusion models, IEKS and the time-dependent field `forced`
(tests/golden/exact_model_*_ld.npz; tests/test_gpu_exact_models.py / tests/test_exact_models_emul.py).
Each line carries "source": "device" or "emulation" and the oracle's distances the ratios are measured in."""
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]


def small_lines(source):
    import _exact_cases as X

    def emit(fixture, kernels, fx, run):
        out = {"fixture": fixture, "kernels": kernels, "source": source, "oracle_distance": X.oracle_distance(fx)}
        try:
            out.update(X.worst_of([X.ratio_record(r) for r in run()]))
        except AssertionError as e:  # a ratio above the bar: the message carries the figures
            out["failed"] = str(e).splitlines()[0]
        print(json.dumps(out), flush=True)

    if source == "emulation":
        import test_exact_emul as T

        for case in X.SMALL_CASES:
            fx = X.load(X.small_name(*case[:4]))
            D = X.SMALL_DIM[case[0]] * (case[2] + 1)
            emit(X.case_id(case), "lane+" + ("lane" if D <= 12 else "rows"), fx, lambda: T.check_emulation(case, "lane"))
            if D <= 16:
                emit(X.case_id(case), "rows+bcast", fx, lambda: T.check_emulation(case, "rows"))
        return
    import odefilters_jl_amd as pkg
    import test_gpu_exact as G

    def setenv(k, v):
        os.environ[k] = v

    for case, filt, smoother in G.COMBOS:
        fx, sol = G.solve_small(pkg, case, filt, smoother, setenv)
        emit(X.case_id(case), f"{filt}+{smoother}", fx, lambda: G.check_small(fx, sol, case, filt, smoother))
    for kind, q in X.LORENZ96_CASES:
        for smoother in ("split", "persistent"):
            fx, sol = G.solve_lorenz96(pkg, kind, q, smoother, setenv)
            emit(f"lorenz96-{kind}{q}", f"mfma+{smoother}", fx, lambda: G.check_lorenz96(fx, sol, kind, q, smoother))


def model_lines(source):
    import _exact_cases as X

    def emit(case, kernels, run):
        fx = X.load(X.model_name(case))
        out = {"fixture": X.model_id(case), "family": case[0], "kernels": kernels, "source": source, "oracle_distance": X.oracle_distance(fx)}
        try:
            out.update(X.worst_of([X.ratio_record(r) for r in run()]))
        except AssertionError as e:  # a ratio above the bar: the message carries the figures
            out["failed"] = str(e).splitlines()[0]
        print(json.dumps(out), flush=True)

    if source == "emulation":
        import test_exact_models_emul as T

        for case in X.MODEL_CASES:
            for kernels in T.emul_kernels(case):
                emit(case, kernels, lambda: T.check_emulation(case, kernels))
        return
    import pytest
    import odefilters_jl_amd as pkg
    import test_gpu_exact_models as G

    mp = pytest.MonkeyPatch()
    for case, filt, smoother in G.MAP_COMBOS:
        with mp.context() as m:
            fx, sol = G.solve_map(pkg, case, filt, smoother, m.setenv)
            emit(case, f"{filt}+{smoother}", lambda: G.check_map(fx, sol, case, filt, smoother))
    for case, filt in G.MV_COMBOS:
        with mp.context() as m:
            fx, sol = G.solve_mv(pkg, case, filt, m.setenv)
            emit(case, f"{filt}+mv", lambda: G.check_mv(fx, sol, case, filt))
    for case, filt in G.IEKS_COMBOS:
        with mp.context() as m:
            fx, sol = G.solve_ieks(pkg, case, filt, m)
            emit(case, filt, lambda: G.check_ieks(fx, sol, case, filt))
            sol.ctx.close()
    for case, filt in G.FORCED_COMBOS:
        with mp.context() as m:
            fx, sol = G.solve_forced(pkg, case, filt, m)
            emit(case, filt, lambda: G.check_forced(fx, sol, case, filt))


if "--models" in sys.argv[1:] or "--models-emul" in sys.argv[1:]:
    model_lines("emulation" if "--models-emul" in sys.argv[1:] else "device")
    sys.exit(0)
if "--small" in sys.argv[1:] or "--small-emul" in sys.argv[1:]:
    small_lines("emulation" if "--small-emul" in sys.argv[1:] else "device")
    sys.exit(0)

import odefilters_jl_amd as pkg
import odefilter_oracle as orc
import _parity as P

GOLD = os.path.join(ROOT, "tests", "golden")
vf = orc.vector_field("pleiades")
for q, kind, tag in ((2, "EK1", ""), (3, "EK0", ""), (5, "EK1", ""), (5, "EK1", "_dt6")):
    fx = np.load(os.path.join(GOLD, f"exact_pleiades_{kind.lower()}q{q}{tag}_smooth_ld.npz"))
    ns, dt = int(fx["nsteps"]), float(fx["dt"])
    D = 28 * (q + 1)
    il = np.tril_indices(D)
    for kernels in ("mfma+split", "mfma+persistent", "tiles+split"):
        filt, smoother = kernels.split("+")
        os.environ["ODEF_PLEIADES_FILTER"] = "tiles" if filt == "tiles" else ""
        os.environ["ODEF_SMOOTH_SPLIT"] = "1" if smoother == "split" else "0"
        ens = pkg.EnsembleProblem(pkg.ODEProblem("pleiades", vf.u0, (0.0, ns * dt), ()), perturb_scale=1e-3, n_perturbed=14)
        alg = (pkg.EK1 if kind == "EK1" else pkg.EK0)(order=q, smooth=True)
        sol = pkg.solve(ens, alg, pkg.EnsembleHIP(), trajectories=5, dt=dt, adaptive=False)
        out = {"fixture": f"{kind}({q}){tag}", "dt": dt, "kernels": kernels}
        for name, mean, cov, rec in (("filt", sol.x_filt_mean(), sol.x_filt_cov(), ns), ("smooth", sol.x_smooth_mean(), sol.x_smooth_cov(), 1)):
            yard_b = np.maximum(fx["oracle_block_err_" + name].max(axis=0), 1e-16)
            yard_c = float(fx["oracle_cov_err_" + name].max())
            rb, rc = [], []
            for k, i in enumerate(fx["trajs"]):
                rb.append(P.block_err(mean[i], fx["mean_" + name][k], 28) / yard_b)
                ec = np.zeros((D, D)); ec[il] = fx[f"cov_{name}_tril"][k]; ec = ec + np.tril(ec, -1).T
                rc.append(P.cov_err(cov[i][rec][None], ec[None]) / yard_c)
            out[name] = {"block_ratio": [round(float(x), 2) for x in np.max(rb, axis=0)], "cov_ratio": round(float(max(rc)), 2),
                         "oracle_block_err": [float(f"{x:.2e}") for x in yard_b], "oracle_cov_err": float(f"{yard_c:.2e}")}
        print(json.dumps(out), flush=True)
