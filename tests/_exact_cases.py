"""The cases of the extended-precision fixtures of `make_exact.py --small` and `--models`, and which kernel families the launchers
can select for each: shared by the generator (tests/golden/make_exact.py), the emulation tests (test_exact_emul.py,
test_exact_models_emul.py), the GPU tests (test_gpu_exact.py, test_gpu_exact_models.py) and tools/exact_ratios.py."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# The small-state kernels (one lane or one 16-lane team per trajectory, D <= 18): field, method, order, diffusion model, step.
# Between them: D = 4, 6, 8, 9, 10, 12, 15, 18; orders 1 ... 5; EK0 and EK1; d = 2 and 3; the static diffusion model; and twice a
# step that is no power of two (the save times np.arange(65) * dt then differ by steps that are not all the same float64).
SMALL_CASES = [
    ("fhn", "EK0", 1, "dynamic", 2.0**-7),
    ("fhn", "EK1", 3, "dynamic", 2.0**-7),
    ("lotka_volterra", "EK1", 2, "dynamic", 2.0**-7),
    ("lotka_volterra", "EK1", 2, "fixed", 2.0**-7),
    ("lotka_volterra", "EK0", 4, "dynamic", 2.0**-6),
    ("vanderpol", "EK0", 3, "dynamic", 1e-2),
    ("vanderpol", "EK1", 4, "dynamic", 2.0**-7),
    ("vanderpol", "EK1", 5, "dynamic", 2.0**-6),
    ("linear", "EK1", 2, "dynamic", 1e-2),
    ("lorenz63", "EK1", 1, "dynamic", 2.0**-7),
    ("lorenz63", "EK0", 2, "dynamic", 2.0**-9),
    ("lorenz63", "EK1", 4, "dynamic", 2.0**-8),
    ("lorenz63", "EK1", 5, "dynamic", 2.0**-8),
]
SMALL_NSTEPS, SMALL_NTRAJ = 64, 4
SMALL_DIM = {"fhn": 2, "lotka_volterra": 2, "vanderpol": 2, "linear": 2, "lorenz63": 3}
RHS_STRUCT = {"fhn": "RhsFHN", "lotka_volterra": "RhsLotkaVolterra", "vanderpol": "RhsVanDerPol", "linear": "RhsLinear",
              "lorenz63": "RhsLorenz63"}

# Lorenz-96 (d = 16) on the matrix-core kernels: the cases, step and ensemble of tests/test_gpu_parity.py
# test_lorenz96_on_the_matrix_core_kernels (12 steps of dt = 2^-7, trajectories 0 and 5 of 6)
LORENZ96_CASES = [("EK1", 2), ("EK1", 3), ("EK0", 3), ("EK1", 5)]


# The families that have kernels, launch paths or arithmetic of their own beside the ones above (make_exact.py --models): family,
# field, method, order, diffusion model, step.  The layout of the small fixtures (4 trajectories, 64 steps, covariances of every
# record); MV diffusions are [traj, step, d].  "map": the on-line MAP update of the global diffusion (ek_math.h, fixed_diffusion
# == 2).  "mv": the diagonal models of EK0 (filter_fixed_lane<..., MV = true>, rts_smooth_mv_kernel, fixed_diffusion == 3 / 4).
# "ieks": the THIRD iteration of solve_ieks, each iteration linearised at the previous one's smoothed u as a float64 record.
# "forced": the time-dependent field of tests/_time_reference.py on the save times t0 + np.arange(65) * dt, t0 = 0.25.
# Not admissible (the oracle's diffusions further than 1e-4 from the extended-precision ones): see DESIGN.md section 4.
MODEL_T0 = 0.25
MODEL_CASES = [
    ("map", "lotka_volterra", "EK1", 2, "fixedMAP", 2.0**-7),
    ("map", "lorenz63", "EK1", 3, "fixedMAP", 2.0**-8),
    ("map", "vanderpol", "EK0", 5, "fixedMAP", 2.0**-6),
    ("mv", "fhn", "EK0", 1, "dynamicMV", 2.0**-7),
    ("mv", "lorenz63", "EK0", 3, "dynamicMV", 2.0**-8),
    ("mv", "vanderpol", "EK0", 5, "dynamicMV", 2.0**-6),
    ("mv", "lorenz63", "EK0", 3, "fixedMV", 2.0**-8),
    ("mv", "fhn", "EK0", 3, "fixedMV", 2.0**-7),
    ("mv", "lotka_volterra", "EK0", 5, "fixedMV", 2.0**-6),
    ("forced", "forced", "EK0", 2, "dynamic", 2.0**-6),
    ("forced", "forced", "EK1", 3, "dynamic", 2.0**-6),
    ("forced", "forced", "EK1", 1, "dynamic", 2.0**-6),
    ("ieks", "lorenz63", "EK1", 3, "dynamic", 2.0**-8),
    ("ieks", "lotka_volterra", "EK1", 2, "fixed", 2.0**-7),
    ("ieks", "vanderpol", "EK1", 4, "fixedMAP", 2.0**-7),
]
MODEL_DIM = {**SMALL_DIM, "forced": 2}
MODEL_RHS_STRUCT = {**RHS_STRUCT, "forced": "RhsForced"}
IEKS_ITERATIONS = 3


def model_cases(family):
    return [c for c in MODEL_CASES if c[0] == family]


def model_id(case):
    family, rhs, kind, q, diffusion, _ = case
    return f"{'ieks-' if family == 'ieks' else ''}{rhs}-{kind}{q}" + ("" if diffusion == "dynamic" else "-" + diffusion)


def model_name(case):
    family, rhs, kind, q, diffusion, _ = case
    return (f"exact_model_{'ieks_' if family == 'ieks' else ''}{rhs}_{kind.lower()}q{q}"
            f"{'' if diffusion == 'dynamic' else '_' + diffusion.lower()}_ld")


def model_grid(case):
    """The documented save times of a MODEL_CASES fixture."""
    return (MODEL_T0 if case[0] == "forced" else 0.0) + np.arange(SMALL_NSTEPS + 1) * case[5]


def model_field(case):
    """The oracle's vector field of a case (`forced` lives in tests/_time_reference.py)."""
    import odefilter_oracle as orc

    if case[1] == "forced":
        import _time_reference as tr

        return tr.forced()
    return orc.vector_field(case[1])


def case_id(case):
    rhs, kind, q, diffusion, _ = case
    return f"{rhs}-{kind}{q}" + ("-fixed" if diffusion == "fixed" else "")


def small_name(rhs, kind, q, diffusion):
    return f"exact_small_{rhs}_{kind.lower()}q{q}{'_fixed' if diffusion == 'fixed' else ''}_ld"


def lorenz96_name(kind, q):
    return f"exact_lorenz96_{kind.lower()}q{q}_smooth_ld"


def load(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


# Which kernels the launchers can select for a state dimension D (csrc/ek_kernels.h LaunchFilterT / LaunchSmoothT, csrc/rows_launch.h;
# DESIGN 3.8), the launch-time overrides that force each, and what odef_kernel_name then reports.
#   filter:   16 lanes per trajectory for D <= 16 below ODEF_FILTER_ROWS_MAX_N trajectories, else one lane per trajectory
#   smoother: DPP row teams for D <= 16 below ODEF_SMOOTH_ROWS_MAX_N; else one lane per trajectory for D <= 12 from
#             ODEF_SMOOTH_LANE_MIN_N on; else LDS row teams (D <= 32)
FILTER_ENV = {"lane": {"ODEF_FILTER_ROWS_MAX_N": "0"}, "rows": {"ODEF_FILTER_ROWS_MAX_N": "1000000000"}}
SMOOTH_ENV = {"lane": {"ODEF_SMOOTH_ROWS_MAX_N": "0", "ODEF_SMOOTH_LANE_MIN_N": "1"},
              "rows": {"ODEF_SMOOTH_ROWS_MAX_N": "0", "ODEF_SMOOTH_LANE_MIN_N": "1000000000"},
              "bcast": {"ODEF_SMOOTH_ROWS_MAX_N": "1000000000", "ODEF_SMOOTH_LANE_MIN_N": "1"}}


def filter_families(D):
    return ["lane", "rows"] if D <= 16 else ["lane"]


def smoother_families(D):
    return (["lane"] if D <= 12 else []) + ["rows"] + (["bcast"] if D <= 16 else [])


def filter_kernel_name(family, rhs, q, ek1):
    tf = "true" if ek1 else "false"
    return (f"odef::ek_filter_fixed_kernel<odef::{RHS_STRUCT[rhs]}, {q}, {tf}, true, " if family == "lane"
            else f"odef::ek_filter_rows_kernel<odef::{RHS_STRUCT[rhs]}, {q}, {tf}, true>")


def smoother_kernel_name(family, d, q):
    return {"lane": f"odef::rts_smooth_lane_kernel<{d}, {q}, false>", "rows": f"odef::rts_smooth_kernel<{d}, {q}>",
            "bcast": f"odef::rts_smooth_bcast_kernel<{d}, {q}, false>"}[family]


def ratio_record(r):
    """The ratios check_against_exact_floored returns, as plain numbers for a JSON line."""
    out = {}
    for name in ("filt", "smooth"):
        out[name] = {"block_ratio": [round(float(x), 2) for x in r[name][0]], "cov_ratio": round(float(r[name][1]), 2)}
    for name in ("diffusion", "loglik"):
        if name in r:
            out[name + "_ratio"] = round(float(r[name]), 2)
    return out


def worst_of(records):
    """Element-wise largest of several ratio_record()s (the trajectories of one run)."""
    out = {}
    for name in ("filt", "smooth"):
        out[name] = {"block_ratio": [max(x) for x in zip(*(r[name]["block_ratio"] for r in records))],
                     "cov_ratio": max(r[name]["cov_ratio"] for r in records)}
    for name in ("diffusion_ratio", "loglik_ratio"):
        if all(name in r for r in records):
            out[name] = max(r[name] for r in records)
    return out


def oracle_distance(fx):
    """The yardsticks of a fixture: the oracle's largest distance from the exact result over the fixture's trajectories."""
    f = lambda x: float(f"{float(x):.2e}")  # noqa: E731
    out = {"floor": f(int(fx["nsteps"]) * 2.0**-52)}
    for name in ("filt", "smooth"):
        out[name] = {"block": [f(x) for x in fx["oracle_block_err_" + name].max(axis=0)], "cov": f(fx["oracle_cov_err_" + name].max())}
    out["diffusion"] = f(np.max(fx["oracle_diffusion_err"]))
    if "oracle_loglik_err" in fx.files and np.isfinite(fx["oracle_loglik_err"]).all():
        out["loglik"] = f(np.max(fx["oracle_loglik_err"]))
    return out
