"""Host-side mirror of the reference's solver interface for the ensemble hot path.

The reference is Julia (`solve(prob, EK1(order=3); adaptive, dt, abstol, reltol)`,
src/algorithms.jl:23-51, src/solution.jl:8-24); there is no Julia toolchain in this image,
so the host side above the C ABI (include/odefilter.h) is written in Python with the same
names, keyword meanings and error behaviour.  `julia/ODEFilterHIP.jl` is the `ccall`
binding a maintainer of the reference would add.

Everything numerical happens in libodefilter_hip.so (HIP kernels for gfx950).  There is no
CPU path: if the library is missing or no GPU is present, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# ODEFILTER_HIP_LIB: development override to A/B-test another build of the same library
LIB_PATH = os.environ.get("ODEFILTER_HIP_LIB") or os.path.join(_HERE, "lib", "libodefilter_hip.so")

# ---- enums (include/odefilter.h) ---------------------------------------------------------
EK0_ID, EK1_ID, IEKS_ID = 0, 1, 2
DIFFUSION = {"dynamic": 0, "fixed": 1, "fixedMAP": 2, "dynamicMV": 3, "fixedMV": 4}
# the diagonal ("multivariate") models: one diffusion per state component, EK0 on the lane kernels only (include/odefilter.h)
MV_DIFFUSIONS = ("dynamicMV", "fixedMV")
RHS = {"fhn": 0, "lorenz63": 1, "lotka_volterra": 2, "vanderpol": 3, "linear": 4, "pleiades": 5, "lorenz96": 6,
       "forced": 7}
RHS_DIMS = {"fhn": (2, 3), "lorenz63": (3, 3), "lotka_volterra": (2, 4), "vanderpol": (2, 1), "linear": (2, 2),
            "pleiades": (28, 0), "lorenz96": (16, 1), "forced": (2, 3)}
SAVE_FINAL, SAVE_EVERYSTEP = 0, 1
RETCODES = {0: "Success", 1: "MaxIters", 2: "DtLessThanMin", 3: "Unstable", 4: "Unstable"}
(F_MEAN, F_COV_TRIL, F_DIFFUSION, F_T, F_LOGLIK, F_NACCEPT, F_NREJECT, F_NF, F_NJAC, F_NSAVED, F_RETCODE,
 F_SMOOTH_MEAN, F_SMOOTH_COV_TRIL, F_U0, F_DENSE_MEAN, F_DENSE_COV_TRIL, F_SAMPLES, F_LINEARIZE_AT) = range(18)
ODEF_F_LINEARIZE_AT = F_LINEARIZE_AT  # IEKS linearisation points [n_save][d][N] (include/odefilter.h)
_INT_FIELDS = {F_NACCEPT, F_NREJECT, F_NF, F_NJAC, F_NSAVED, F_RETCODE}
# ensemble summary per time (odef_summary_field, include/odefilter.h): id = S_BASE + 8 * source + quantity
S_BASE = 64
S_SOURCE_FILTER, S_SOURCE_SMOOTH, S_SOURCE_DENSE = 0, 1, 2
S_COUNT, S_MEAN, S_COV_WITHIN, S_COV_BETWEEN = 0, 1, 2, 3
SUMMARY_FIELDS = {
    "ODEF_S_BASE": 64,
    "ODEF_S_FILTER_COUNT": 64, "ODEF_S_FILTER_MEAN": 65, "ODEF_S_FILTER_COV_WITHIN": 66, "ODEF_S_FILTER_COV_BETWEEN": 67,
    "ODEF_S_SMOOTH_COUNT": 72, "ODEF_S_SMOOTH_MEAN": 73, "ODEF_S_SMOOTH_COV_WITHIN": 74, "ODEF_S_SMOOTH_COV_BETWEEN": 75,
    "ODEF_S_DENSE_COUNT": 80, "ODEF_S_DENSE_MEAN": 81, "ODEF_S_DENSE_COV_WITHIN": 82, "ODEF_S_DENSE_COV_BETWEEN": 83,
}


def summary_field(source: int, quantity: int) -> int:
    """Field id of an ensemble-summary array: source 0 filter / 1 smoothed / 2 dense records, quantity 0 COUNT / 1 MEAN /
    2 COV_WITHIN / 3 COV_BETWEEN."""
    if source not in (0, 1, 2) or quantity not in (0, 1, 2, 3):
        raise OdefError(f"no ensemble-summary field for source {source}, quantity {quantity}")
    return S_BASE + 8 * source + quantity


def _is_summary_field(f: int) -> bool:
    return S_BASE <= f < S_BASE + 24 and (f - S_BASE) % 8 < 4


# solution errors per trajectory (odef_errors_field, include/odefilter.h): id = E_BASE + 8 * source + quantity
E_BASE = 128
E_SOURCE_FILTER, E_SOURCE_SMOOTH = 0, 1
E_FINAL, E_L2, E_LINF, E_CHI2, E_NUSED, E_U_ANALYTIC = range(6)
E_REFERENCE = 144  # odef_bind_device only: the truth [n_save][d][N] in device memory
ERRORS_FIELDS = {
    "ODEF_E_BASE": 128,
    "ODEF_E_FINAL": 128, "ODEF_E_L2": 129, "ODEF_E_LINF": 130, "ODEF_E_CHI2": 131, "ODEF_E_NUSED": 132, "ODEF_E_U_ANALYTIC": 133,
    "ODEF_E_SMOOTH_FINAL": 136, "ODEF_E_SMOOTH_L2": 137, "ODEF_E_SMOOTH_LINF": 138, "ODEF_E_SMOOTH_CHI2": 139,
    "ODEF_E_SMOOTH_NUSED": 140, "ODEF_E_SMOOTH_U_ANALYTIC": 141,
    "ODEF_E_REFERENCE": 144,
}
_NO_TRUTH = "nothing to compare with"  # the library's refusal for a field without `analytic` and no bound reference


def errors_field(source: int, quantity: int) -> int:
    """Field id of a solution-error array: source 0 filter / 1 smoothed records, quantity 0 FINAL / 1 L2 / 2 LINF / 3 CHI2 /
    4 NUSED / 5 U_ANALYTIC."""
    if source not in (0, 1) or quantity not in range(6):
        raise OdefError(f"no solution-error field for source {source}, quantity {quantity}")
    return E_BASE + 8 * source + quantity


def _is_errors_field(f: int) -> bool:
    return E_BASE <= f < E_BASE + 16 and (f - E_BASE) % 8 < 6


# data log-likelihood of noisy observations per trajectory (odef_data_field, include/odefilter.h)
L_BASE = 192
L_DATA_LOGLIK, L_DATA_MAHALANOBIS = 192, 193
L_OBS_SAVE, L_OBS_COMPONENT, L_OBS_VALUE, L_OBS_NOISE = 200, 201, 202, 203  # odef_bind_device only
DATA_FIELDS = {
    "ODEF_L_BASE": 192,
    "ODEF_L_DATA_LOGLIK": 192, "ODEF_L_DATA_MAHALANOBIS": 193,
    "ODEF_L_OBS_SAVE": 200, "ODEF_L_OBS_COMPONENT": 201, "ODEF_L_OBS_VALUE": 202, "ODEF_L_OBS_NOISE": 203,
}
L_OBS_TIME = 204  # odef_bind_device only: observation times instead of save indices (fixed and adaptive grids)
DATA_TIME_FIELDS = {"ODEF_L_OBS_TIME": 204}
K_DATA_LOGLIK = 4  # `which` of odef_kernel_time_ms / odef_kernel_name

# event location per trajectory (odef_event_field, include/odefilter.h): id = EV_BASE + 8 * source + quantity
EV_BASE = 256
EV_SOURCE_FILTER, EV_SOURCE_SMOOTH = 0, 1
EV_COUNT, EV_TIME, EV_TIME_VAR, EV_U, EV_DIRECTION, EV_SAVE, EV_NEVAL = range(7)
EV_SPEC, EV_LEVEL = 280, 281  # odef_bind_device only
EVENT_FIELDS = {
    "ODEF_EV_BASE": 256,
    "ODEF_EV_COUNT": 256, "ODEF_EV_TIME": 257, "ODEF_EV_TIME_VAR": 258, "ODEF_EV_U": 259, "ODEF_EV_DIRECTION": 260,
    "ODEF_EV_SAVE": 261, "ODEF_EV_NEVAL": 262,
    "ODEF_EV_SMOOTH_COUNT": 264, "ODEF_EV_SMOOTH_TIME": 265, "ODEF_EV_SMOOTH_TIME_VAR": 266, "ODEF_EV_SMOOTH_U": 267,
    "ODEF_EV_SMOOTH_DIRECTION": 268, "ODEF_EV_SMOOTH_SAVE": 269, "ODEF_EV_SMOOTH_NEVAL": 270,
    "ODEF_EV_SPEC": 280, "ODEF_EV_LEVEL": 281,
}
K_EVENTS = 5  # `which` of odef_kernel_time_ms / odef_kernel_name


def event_field(source: int, quantity: int) -> int:
    """Field id of an event array: source 0 filter / 1 smoothed posterior, quantity 0 COUNT / 1 TIME / 2 TIME_VAR / 3 U /
    4 DIRECTION / 5 SAVE / 6 NEVAL."""
    if source not in (0, 1) or quantity not in range(7):
        raise OdefError(f"no event field for source {source}, quantity {quantity}")
    return EV_BASE + 8 * source + quantity


def _is_event_field(f: int) -> bool:
    return EV_BASE <= f < EV_BASE + 16 and (f - EV_BASE) % 8 < 7


# ensemble quantiles per time (odef_quantile_field, include/odefilter.h): id = Q_BASE + 8 * source + quantity
Q_BASE = 320
Q_QUANTILES, Q_COUNT = 0, 1
Q_PROBS = 344  # odef_bind_device only: the probabilities double [P] in device memory
QUANTILE_FIELDS = {
    "ODEF_Q_BASE": 320,
    "ODEF_Q_FILTER": 320, "ODEF_Q_COUNT_FILTER": 321,
    "ODEF_Q_SMOOTH": 328, "ODEF_Q_COUNT_SMOOTH": 329,
    "ODEF_Q_DENSE": 336, "ODEF_Q_COUNT_DENSE": 337,
    "ODEF_Q_PROBS": 344,
}
K_QUANTILES = 6  # `which` of odef_kernel_time_ms / odef_kernel_name


def quantile_field(source: int, quantity: int) -> int:
    """Field id of an ensemble-quantile array: source 0 filter / 1 smoothed / 2 dense records, quantity 0 the quantiles
    [n_t, P, d] / 1 the count [n_t]."""
    if source not in (0, 1, 2) or quantity not in (0, 1):
        raise OdefError(f"no ensemble-quantile field for source {source}, quantity {quantity}")
    return Q_BASE + 8 * source + quantity


def _is_quantile_field(f: int) -> bool:
    return Q_BASE <= f < Q_BASE + 24 and (f - Q_BASE) % 8 < 2


# weighted ensemble summary per time (odef_wsummary_field, include/odefilter.h): id = W_BASE + 8 * source + quantity
W_BASE = 384
W_COUNT, W_MEAN, W_COV_WITHIN, W_COV_BETWEEN, W_LOG_EVIDENCE, W_ESS = range(6)
W_LOGWEIGHT = 408  # odef_bind_device only: the unnormalised log-weights double [N] in device memory
_W_QUANTITIES = ("COUNT", "MEAN", "COV_WITHIN", "COV_BETWEEN", "LOG_EVIDENCE", "ESS")
WSUMMARY_FIELDS = {"ODEF_W_BASE": 384, "ODEF_W_LOGWEIGHT": 408}
WSUMMARY_FIELDS.update({f"ODEF_W_{src}_{name}": 384 + 8 * s + q
                        for s, src in enumerate(("FILTER", "SMOOTH", "DENSE")) for q, name in enumerate(_W_QUANTITIES)})
K_WSUMMARY = 7  # `which` of odef_kernel_time_ms / odef_kernel_name


def wsummary_field(source: int, quantity: int) -> int:
    """Field id of a weighted-summary array: source 0 filter / 1 smoothed / 2 dense records, quantity 0 COUNT / 1 MEAN /
    2 COV_WITHIN / 3 COV_BETWEEN / 4 LOG_EVIDENCE / 5 ESS."""
    if source not in (0, 1, 2) or quantity not in range(6):
        raise OdefError(f"no weighted-summary field for source {source}, quantity {quantity}")
    return W_BASE + 8 * source + quantity


def _is_wsummary_field(f: int) -> bool:
    return W_BASE <= f < W_BASE + 24 and (f - W_BASE) % 8 < 6

# dtype and shape (of a Context `c`) of every derived field, by family and quantity; the source does not matter
_FLAT = lambda c: (-1,)  # noqa: E731  ([n_t] counts, [N] per-trajectory values)
_DERIVED_LAYOUT = {
    ("summary", S_COUNT): (np.int64, _FLAT),
    ("summary", S_MEAN): (np.float64, lambda c: (-1, c.d)),
    ("summary", S_COV_WITHIN): (np.float64, lambda c: (-1, c.d * (c.d + 1) // 2)),
    ("summary", S_COV_BETWEEN): (np.float64, lambda c: (-1, c.d * (c.d + 1) // 2)),
    ("errors", E_FINAL): (np.float64, _FLAT), ("errors", E_L2): (np.float64, _FLAT),
    ("errors", E_LINF): (np.float64, _FLAT), ("errors", E_CHI2): (np.float64, _FLAT),
    ("errors", E_NUSED): (np.int64, _FLAT),
    ("errors", E_U_ANALYTIC): (np.float64, lambda c: (-1, c.d, c.N)),
    ("data", L_DATA_LOGLIK - L_BASE): (np.float64, _FLAT), ("data", L_DATA_MAHALANOBIS - L_BASE): (np.float64, _FLAT),
    ("event", EV_COUNT): (np.int32, _FLAT),
    ("event", EV_TIME): (np.float64, lambda c: (-1, c.N)), ("event", EV_TIME_VAR): (np.float64, lambda c: (-1, c.N)),
    ("event", EV_U): (np.float64, lambda c: (-1, c.d, c.N)),
    ("event", EV_DIRECTION): (np.int32, lambda c: (-1, c.N)), ("event", EV_SAVE): (np.int32, lambda c: (-1, c.N)),
    ("event", EV_NEVAL): (np.int32, lambda c: (-1, c.N)),
}
_DERIVED = {S_BASE + 8 * s + q: _DERIVED_LAYOUT["summary", q] for s in range(3) for q in range(4)}
_DERIVED.update({E_BASE + 8 * s + q: _DERIVED_LAYOUT["errors", q] for s in range(2) for q in range(6)})
_DERIVED.update({L_BASE + q: _DERIVED_LAYOUT["data", q] for q in range(2)})
_DERIVED.update({EV_BASE + 8 * s + q: _DERIVED_LAYOUT["event", q] for s in range(2) for q in range(7)})
# quantiles [n_t, P, d]: P is that of the bound probabilities, so it follows from the flat size and the source's count [n_t]
_DERIVED.update({Q_BASE + 8 * s + Q_QUANTILES: (np.float64, lambda c, s=s: (c.field_bytes(Q_BASE + 8 * s + Q_COUNT) // 8, -1, c.d))
                 for s in range(3)})
_DERIVED.update({Q_BASE + 8 * s + Q_COUNT: (np.int64, _FLAT) for s in range(3)})
# weighted summary: the four arrays of the summary, then LOG_EVIDENCE and ESS [n_t]
_DERIVED.update({W_BASE + 8 * s + q: _DERIVED_LAYOUT["summary", q] for s in range(3) for q in range(4)})
_DERIVED.update({W_BASE + 8 * s + q: (np.float64, _FLAT) for s in range(3) for q in (W_LOG_EVIDENCE, W_ESS)})


def _fetch(lib, h, f: int, dtype=None) -> np.ndarray:
    """Field `f` of the context handle `h` as a flat array: byte count, allocation, `odef_get`.  A refusal raises OdefError with
    the library's message.  dtype: that of the field unless given."""
    if dtype is None:
        dtype = _DERIVED[f][0] if f in _DERIVED else np.int32 if f in _INT_FIELDS else np.float64
    b = C.c_size_t()
    if lib.odef_field_bytes(h, f, C.byref(b)) != 0:
        raise OdefError(lib.odef_last_error(h).decode() or f"odef_field_bytes failed for field {f}")
    out = np.empty(b.value // np.dtype(dtype).itemsize, dtype=dtype)
    if lib.odef_get(h, f, out.ctypes.data_as(_vp), b.value) != 0:
        raise OdefError(lib.odef_last_error(h).decode())
    return out


def _observation_arrays(t, d, N, times, data, noise_var, components):
    """The four inputs of the data log-likelihood in the ABI layout, validated on the host: (saves int64 [M], comps int64 [o],
    values [M, o] or [M, o, N], noise [o], per_trajectory).  `times` must equal entries of the save grid `t` exactly."""
    t = np.asarray(t, np.float64).reshape(-1)
    times = np.atleast_1d(np.asarray(times, np.float64))
    if times.ndim != 1 or times.size == 0:
        raise OdefError("data_loglik: times must be a non-empty 1-d array")
    saves = np.searchsorted(t, times)
    if np.any(saves >= t.size) or np.any(t[np.minimum(saves, t.size - 1)] != times):
        bad = times[(saves >= t.size) | (t[np.minimum(saves, t.size - 1)] != times)]
        raise OdefError(f"data_loglik: observation times must equal save times of the solution exactly; not on the grid: {bad[:4]}")
    if np.any(np.diff(saves) <= 0):
        raise OdefError("data_loglik: observation times must be strictly increasing")
    return (saves.astype(np.int64),) + _observation_values(d, N, saves.size, data, noise_var, components)


def _observation_time_arrays(d, N, times, data, noise_var, components, t0=None, t_last=None):
    """The inputs of the data log-likelihood at arbitrary times in the ABI layout, validated on the host: (times float64 [M],
    comps int64 [o], values [M, o] or [M, o, N], noise [o], per_trajectory).  `t0`: the first save time; `t_last`: the last save
    time of a fixed grid (an adaptive solve ends per trajectory: a time above a trajectory's own last save gives NaN there)."""
    times = np.atleast_1d(np.asarray(times, np.float64))
    if times.ndim != 1 or times.size == 0:
        raise OdefError("data_loglik: times must be a non-empty 1-d array")
    if not np.all(np.isfinite(times)):
        raise OdefError("data_loglik: observation times must be finite")
    if np.any(np.diff(times) <= 0):
        raise OdefError("data_loglik: observation times must be strictly increasing")
    if t0 is not None and times[0] < t0:
        raise OdefError(f"data_loglik: observation time {times[0]!r} lies before the first save t0 = {t0!r}")
    if t_last is not None and times[-1] > t_last:
        raise OdefError(f"data_loglik: observation time {times[-1]!r} lies above the last save of the grid, {t_last!r} (a time meant "
                        "as that save must equal it exactly)")
    return (np.ascontiguousarray(times),) + _observation_values(d, N, times.size, data, noise_var, components)


def _on_grid(t, times) -> bool:
    """True when every entry of `times` equals an entry of the fixed save grid `t` exactly."""
    t = np.asarray(t, np.float64).reshape(-1)
    times = np.atleast_1d(np.asarray(times, np.float64))
    if times.ndim != 1 or times.size == 0 or t.size == 0:
        return True  # (left to the validation of the save path)
    k = np.minimum(np.searchsorted(t, times), t.size - 1)
    return bool(np.all(t[k] == times))


def _observation_values(d, N, M, data, noise_var, components):
    """(comps int64 [o], values [M, o] or [M, o, N], noise [o], per_trajectory) of M observations, validated."""
    comps = np.arange(d) if components is None else np.atleast_1d(np.asarray(components))
    if comps.ndim != 1 or comps.size == 0 or not np.issubdtype(comps.dtype, np.integer):
        raise OdefError("data_loglik: components must be a non-empty 1-d integer array")
    if np.any(comps < 0) or np.any(comps >= d) or np.any(np.diff(comps) <= 0):
        raise OdefError(f"data_loglik: components must be strictly increasing within 0 .. {d - 1}")
    o = comps.size
    data = np.asarray(data, np.float64)
    if data.shape == (M, o):
        per_traj, values = False, np.ascontiguousarray(data)
    elif data.shape == (N, M, o):
        per_traj, values = True, np.ascontiguousarray(data.transpose(1, 2, 0))
    else:
        raise OdefError(f"data_loglik: data must have shape ({M}, {o}) or ({N}, {M}, {o}), got {data.shape}")
    noise = np.asarray(noise_var, np.float64)
    if noise.ndim == 0:
        noise = np.full(o, float(noise))
    if noise.shape != (o,):
        raise OdefError(f"data_loglik: noise_var must be a scalar or have shape ({o},), got {noise.shape}")
    if not np.all(np.isfinite(noise)) or np.any(noise <= 0):
        raise OdefError("data_loglik: noise variances must be finite and positive")
    return comps.astype(np.int64), values, np.ascontiguousarray(noise), per_traj


@dataclass
class Events:
    """Located level crossings per trajectory (`EnsembleSolution.events`), trajectory-major.  `count [N]` is the number of
    crossings of the whole trajectory and may exceed the K = `max_events` slots; slot s < min(count, K) of trajectory i holds the
    time `t[i, s]`, its standard deviation `t_std[i, s]` (sqrt of Var u_c(t*) / E[u'_c(t*)]^2), the solution `u[i, s, :]` there, the
    `direction` (+1 up, -1 down), the left save `save` of the step that holds it and the dense evaluations spent, `neval`.
    Unused slots: NaN, direction 0, save -1, neval 0."""
    count: np.ndarray
    t: np.ndarray
    t_std: np.ndarray
    u: np.ndarray
    direction: np.ndarray
    save: np.ndarray
    neval: np.ndarray

    @classmethod
    def from_abi(cls, a):
        """From the seven ABI arrays (count [N], time / var [K, N], u [K, d, N], direction / save / neval [K, N])."""
        count, time, var, u, direction, save, neval = a
        with np.errstate(invalid="ignore"):
            std = np.sqrt(var.T)
        return cls(count, np.ascontiguousarray(time.T), np.ascontiguousarray(std), np.ascontiguousarray(u.transpose(2, 0, 1)),
                   np.ascontiguousarray(direction.T), np.ascontiguousarray(save.T), np.ascontiguousarray(neval.T))

    @classmethod
    def concatenate(cls, parts):
        return cls(*(np.concatenate([getattr(p, k) for p in parts]) for k in ("count", "t", "t_std", "u", "direction", "save", "neval")))


def _event_arrays(d, N, component, level, direction, max_events):
    """The two inputs of the event location in the ABI layout, validated on the host: (spec int64 [3], level [1] or [N])."""
    if int(component) != component or not 0 <= int(component) < d:
        raise OdefError(f"events: component must be an integer within 0 .. {d - 1}")
    if direction not in (-1, 0, 1):
        raise OdefError("events: direction must be -1 (down), 0 (both) or +1 (up)")
    if int(max_events) != max_events or int(max_events) < 1:
        raise OdefError("events: max_events must be a positive integer")
    lvl = np.atleast_1d(np.asarray(level, np.float64))
    if lvl.shape not in ((1,), (N,)):
        raise OdefError(f"events: level must be a scalar or have shape ({N},), got {lvl.shape}")
    return np.array([int(component), int(direction), int(max_events)], np.int64), np.ascontiguousarray(lvl)


def _to_device(arrays, device):
    """numpy arrays -> torch tensors on GPU `device` (kept alive by the caller while they are bound).  A process that uses this
    brings up torch's HIP runtime before the library's first context (`torch.cuda.init()`), as tests/conftest.py does: brought up
    second it has been seen to find no GPU."""
    import torch

    dev = torch.device("cuda", int(device) if device >= 0 else torch.cuda.current_device())
    out = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]
    torch.cuda.synchronize(dev)
    return out
MAX_ORDER = 5


class OdefConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("alg", C.c_int32), ("order", C.c_int32), ("diffusion", C.c_int32),
        ("smooth", C.c_int32), ("rhs_id", C.c_int32), ("d", C.c_int32), ("n_params", C.c_int32),
        ("params_shared", C.c_int32), ("save_mode", C.c_int32), ("device", C.c_int32), ("want_loglik", C.c_int32),
        ("n_traj", C.c_int64),
    ]


class OdefController(C.Structure):
    _fields_ = [(n, C.c_double) for n in
                ("beta1", "beta2", "gamma", "qmin", "qmax", "qsteady_min", "qsteady_max", "qoldinit", "dtmin", "dtmax")]


# every symbol include/odefilter.h declares: name -> (restype, argtypes)
_dp = C.POINTER(C.c_double)
_vp = C.c_void_p
SYMBOLS = {
    "odef_version": (C.c_int, []),
    "odef_last_error": (C.c_char_p, [_vp]),
    "odef_create": (C.c_int, [C.POINTER(_vp), C.POINTER(OdefConfig)]),
    "odef_rhs_compile": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_char_p, C.POINTER(C.c_int32)]),
    "odef_destroy": (None, [_vp]),
    "odef_set_stream": (C.c_int, [_vp, _vp]),
    "odef_set_problem": (C.c_int, [_vp, _dp, _dp, C.c_double]),
    "odef_set_problem_device": (C.c_int, [_vp, _vp, _vp, C.c_double]),
    "odef_set_problem_perturbed": (C.c_int, [_vp, _dp, _dp, C.c_double, C.c_double, C.c_uint64, C.c_int64, C.c_int32]),
    "odef_solve_fixed": (C.c_int, [_vp, _dp, C.c_int64]),
    "odef_solve_adaptive": (C.c_int, [_vp, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(OdefController), C.c_int64]),
    "odef_smooth": (C.c_int, [_vp]),
    "odef_dense_output": (C.c_int, [_vp, _dp, C.c_int64, C.c_int]),
    "odef_sample": (C.c_int, [_vp, C.c_int64, C.c_uint64, C.c_double]),
    "odef_dense_sample": (C.c_int, [_vp, C.POINTER(C.c_double), C.c_int64, C.c_int64, C.c_uint64, C.c_double]),
    "odef_n_save": (C.c_int64, [_vp]),
    "odef_field_bytes": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_size_t)]),
    "odef_get": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t]),
    "odef_get_device": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "odef_bind_device": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t]),
    "odef_synchronize": (C.c_int, [_vp]),
    "odef_kernel_time_ms": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "odef_kernel_name": (C.c_int, [_vp, C.c_int, C.c_char_p, C.c_size_t]),
    "odef_ibm": (C.c_int, [C.c_int, C.c_int, _dp, _dp]),
    "odef_preconditioner": (C.c_int, [C.c_int, C.c_int, C.c_double, _dp]),
    "odef_predict": (C.c_int, [C.c_int, C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp]),
    "odef_update": (C.c_int, [C.c_int, C.c_int, C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp]),
    "odef_smooth_step": (C.c_int, [C.c_int, C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    # ensemble sharded over the GPUs of one node by one process
    "odef_shard_range": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "odef_group_layout": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "odef_unpad_gathered": (C.c_int, [_dp, C.c_int32, C.c_int32, C.c_int64, _dp]),
    "odef_group_create": (C.c_int, [C.POINTER(_vp), C.POINTER(OdefConfig), C.c_int32, C.POINTER(C.c_int32)]),
    "odef_group_destroy": (None, [_vp]),
    "odef_group_last_error": (C.c_char_p, [_vp]),
    "odef_group_size": (C.c_int32, [_vp]),
    "odef_group_ctx": (_vp, [_vp, C.c_int32]),
    "odef_group_shard": (C.c_int, [_vp, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "odef_group_set_problem": (C.c_int, [_vp, _dp, _dp, C.c_double]),
    "odef_group_set_problem_perturbed": (C.c_int, [_vp, _dp, _dp, C.c_double, C.c_double, C.c_uint64, C.c_int32]),
    "odef_group_solve_fixed": (C.c_int, [_vp, _dp, C.c_int64]),
    "odef_group_solve_adaptive": (C.c_int, [_vp, C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(OdefController), C.c_int64]),
    "odef_group_smooth": (C.c_int, [_vp]),
    "odef_allgather": (C.c_int, [_vp, C.c_int]),
    "odef_group_get_gathered": (C.c_int, [_vp, C.c_int32, _dp, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
}

_lib = None


def load_library() -> C.CDLL:
    """Load libodefilter_hip.so; fail loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(make -C odefilters.jl_amd/csrc).  There is no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


class OdefError(RuntimeError):
    pass


def shard_range(n_traj: int, n_shards: int, shard: int):
    """(first, count) of a shard: contiguous blocks, the first n_traj % n_shards one longer (`odef_shard_range`; host
    arithmetic only, works without a GPU)."""
    first, count = C.c_int64(), C.c_int64()
    if load_library().odef_shard_range(int(n_traj), int(n_shards), int(shard), C.byref(first), C.byref(count)) != 0:
        raise OdefError(f"odef_shard_range({n_traj}, {n_shards}, {shard}): invalid arguments")
    return int(first.value), int(count.value)


class DeviceGroup:
    """`odef_group`: one ensemble sharded over the GPUs of a node by THIS process (what a Julia host binds with ccall,
    julia/ODEFilterHIP.jl) -- contiguous blocks, no exchange while stepping, `allgather()` = the one RCCL collective."""

    def __init__(self, rhs: str, order: int, alg: int, n_traj: int, n_devices: int, *, device_ids=None, diffusion="dynamic",
                 smooth=False, save_everystep=True, want_loglik=True, params_shared=True):
        self.lib = load_library()
        d, npar = RHS_DIMS[rhs]
        cfg = OdefConfig()
        cfg.struct_size = C.sizeof(OdefConfig)
        cfg.alg, cfg.order, cfg.diffusion = alg, order, DIFFUSION[diffusion]
        cfg.smooth, cfg.rhs_id, cfg.d, cfg.n_params = int(smooth), RHS[rhs], d, npar
        cfg.params_shared = int(params_shared)  # False: `set_problem` takes p [N, n_params], every shard its rows
        cfg.save_mode = SAVE_EVERYSTEP if (save_everystep or smooth) else SAVE_FINAL
        cfg.device, cfg.want_loglik, cfg.n_traj = -1, int(want_loglik), n_traj
        self.d, self.D, self.N, self.G = d, d * (order + 1), n_traj, n_devices
        self._adaptive = False  # the last solve was adaptive (its T is [n_save][N], its grid per trajectory)
        self.TRI, self.mv = self.D * (self.D + 1) // 2, diffusion in MV_DIFFUSIONS
        ids = (C.c_int32 * n_devices)(*device_ids) if device_ids is not None else None
        h = _vp()
        if self.lib.odef_group_create(C.byref(h), C.byref(cfg), n_devices, ids) != 0:
            raise OdefError(self.lib.odef_group_last_error(None).decode())
        self._h = h
        self._devices = list(device_ids) if device_ids is not None else list(range(n_devices))

    def _chk(self, rc):
        if rc != 0:
            raise OdefError(self.lib.odef_group_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self.lib.odef_group_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def shard(self, g: int):
        first, count = C.c_int64(), C.c_int64()
        self._chk(self.lib.odef_group_shard(self._h, g, C.byref(first), C.byref(count)))
        return int(first.value), int(count.value)

    def set_problem(self, u0, p, t0):
        u0 = np.ascontiguousarray(u0, dtype=np.float64)
        pp = _as_dp(np.ascontiguousarray(p, dtype=np.float64)) if p is not None and len(p) else None
        self._chk(self.lib.odef_group_set_problem(self._h, _as_dp(u0), pp, float(t0)))

    def set_problem_perturbed(self, base_u0, p, t0, scale, seed=0x0DEF17E5, n_perturbed=None):
        base = np.ascontiguousarray(base_u0, dtype=np.float64)
        pp = _as_dp(np.ascontiguousarray(p, dtype=np.float64)) if p is not None and len(p) else None
        self._chk(self.lib.odef_group_set_problem_perturbed(self._h, _as_dp(base), pp, float(t0), float(scale), C.c_uint64(seed),
                                                            self.d if n_perturbed is None else n_perturbed))

    def solve_fixed(self, tgrid):
        tg = np.ascontiguousarray(tgrid, dtype=np.float64)
        self._chk(self.lib.odef_group_solve_fixed(self._h, _as_dp(tg), len(tg)))
        self._adaptive = False

    def solve_adaptive(self, t1, abstol=1e-6, reltol=1e-3, dt0=1e-3, max_steps=4096):
        self._chk(self.lib.odef_group_solve_adaptive(self._h, float(t1), float(abstol), float(reltol), float(dt0), None, int(max_steps)))
        self._adaptive = True

    def smooth(self):
        self._chk(self.lib.odef_group_smooth(self._h))

    def solve_ieks(self, tgrid, iterations=10):
        """`solve_ieks` on every shard (an IEKS group, alg=IEKS_ID): the field of linearisation points starts empty (the first
        iteration is EK1), then each iteration is one fixed-grid solve plus the smoother, whose result the next solve linearises
        at -- all on the devices."""
        if iterations < 1:
            raise OdefError("solve_ieks: iterations must be >= 1")
        for g in range(self.G):
            self._chk_ctx(g, self.lib.odef_bind_device(self.lib.odef_group_ctx(self._h, g), F_LINEARIZE_AT, None, 0))
        for _ in range(int(iterations)):
            self.solve_fixed(tgrid)
            self.smooth()

    def _chk_ctx(self, g, rc):
        if rc != 0:
            raise OdefError(self.lib.odef_last_error(self.lib.odef_group_ctx(self._h, g)).decode())

    def allgather(self, smoothed=False, from_device=0) -> np.ndarray:
        """Final posterior means of the WHOLE ensemble, [D, N], as device `from_device` holds them after the all-gather."""
        self._chk(self.lib.odef_allgather(self._h, int(smoothed)))
        out = np.empty((self.D, self.N))
        self._chk(self.lib.odef_group_get_gathered(self._h, from_device, _as_dp(out), None, None))
        return out

    def gather_field(self, f: int) -> np.ndarray:
        """A per-save or per-trajectory field of the WHOLE ensemble, read shard by shard from the hosts of the shards and
        joined along the trajectory axis: the layout of Context.get for one context of all N trajectories (the d-wide
        DIFFUSION of the MV models included)."""
        parts = []
        for g in range(self.G):
            out = _fetch(self.lib, self.lib.odef_group_ctx(self._h, g), f)
            n = self.shard(g)[1]
            if f in (F_MEAN, F_SMOOTH_MEAN):
                out = out.reshape(-1, self.D, n)
            elif f in (F_COV_TRIL, F_SMOOTH_COV_TRIL):
                out = out.reshape(-1, self.TRI, n)
            elif f == F_DIFFUSION:
                out = out.reshape(-1, self.d, n) if self.mv else out.reshape(-1, n)
            elif f == F_LINEARIZE_AT:
                out = out.reshape(-1, self.d, n)
            parts.append(out)
        return np.concatenate(parts, axis=-1)

    def solution_errors(self, source: int):
        """Solution errors of the WHOLE ensemble (`odef_errors_field`): every shard runs the pass on its own device, the
        per-trajectory arrays are joined along the trajectory axis.  dict with "l∞", "l2", "final", "chi2" [N] and "nused"."""
        parts = [Context._solution_errors(self.lib, self.lib.odef_group_ctx(self._h, g), source) for g in range(self.G)]
        return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}

    def data_loglik(self, times, data, noise_var, components=None):
        """Data log-likelihood of the WHOLE ensemble (`EnsembleSolution.data_loglik`): the same observations go to every shard
        through `odef_group_ctx`, per-trajectory values are split by `odef_group_shard`, every shard runs the pass on its own
        device and the results are joined along the trajectory axis.  Times that all equal saves of a fixed grid go by save
        index, any others and every adaptive solve by time (`bind_observation_times`).  Returns (loglik [N], mahalanobis [N])."""
        adaptive = self._adaptive
        try:
            t = _fetch(self.lib, self.lib.odef_group_ctx(self._h, 0), F_T)
        except OdefError:
            raise OdefError("data_loglik: needs a solve first") from None
        by_time = adaptive or not _on_grid(t, times)
        if by_time:
            first, comps, values, noise, per_traj = _observation_time_arrays(self.d, self.N, times, data, noise_var, components,
                                                                             None if adaptive else t[0], None if adaptive else t[-1])
        else:
            first, comps, values, noise, per_traj = _observation_arrays(t, self.d, self.N, times, data, noise_var, components)
        self._obs_bufs = []
        parts = []
        for g in range(self.G):
            lo, count = self.shard(g)
            vals = values[:, :, lo:lo + count] if per_traj else values
            bufs = _to_device((first, comps, vals, noise), self._devices[g])
            self._obs_bufs.append(bufs)
            parts.append(Context._data_loglik(self.lib, self.lib.odef_group_ctx(self._h, g), bufs, by_time))
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])

    def events(self, component, level=0.0, direction=0, max_events=1, smoothed=False) -> "Events":
        """Level crossings of the WHOLE ensemble (`EnsembleSolution.events`): the same spec goes to every shard through
        `odef_group_ctx`, a per-trajectory level is split by `odef_group_shard`, every shard runs the pass on its own device and
        the results are joined along the trajectory axis."""
        spec, lvl = _event_arrays(self.d, self.N, component, level, direction, max_events)
        self._event_bufs = []
        parts = []
        for g in range(self.G):
            first, count = self.shard(g)
            bufs = _to_device((spec, lvl if lvl.size == 1 else lvl[first:first + count]), self._devices[g])
            self._event_bufs.append(bufs)
            parts.append(Context._events(self.lib, self.lib.odef_group_ctx(self._h, g), self, int(bool(smoothed)), bufs))
        return Events.concatenate(parts)

    def ensemble_moments(self, source: int):
        """Ensemble summary of the WHOLE ensemble: every shard reduces its own records on its device (`odef_summary_field`),
        the per-shard blocks (kilobytes) are pooled on the host with `merge_moments`.  Returns (count, mean, within, between)."""
        parts = []
        for g in range(self.G):
            c = self.lib.odef_group_ctx(self._h, g)
            parts.append(tuple(_fetch(self.lib, c, f).reshape(_DERIVED[f][1](self))
                               for f in (summary_field(source, qty) for qty in range(4))))
        return merge_moments(parts)

    def summary(self, smoothed: bool = False) -> "EnsembleSummary":
        """`EnsembleSummary` of the whole ensemble on the save grid of a fixed-grid solve."""
        n, m, w, b = self.ensemble_moments(S_SOURCE_SMOOTH if smoothed else S_SOURCE_FILTER)
        return EnsembleSummary.from_moments(_fetch(self.lib, self.lib.odef_group_ctx(self._h, 0), F_T), n, m, w, b)

    def weighted_moments(self, source: int, log_weights):
        """Weighted ensemble summary of the WHOLE ensemble (`Context.weighted_moments`): `log_weights` [N] is split by
        `odef_group_shard`, every shard binds its block and reduces its own records on its device (`odef_wsummary_field`), the
        per-shard blocks (kilobytes) are pooled on the host with `merge_weighted_moments`.  Returns (count, mean, within, between,
        log_evidence, ess)."""
        w = np.ascontiguousarray(np.asarray(log_weights, float).reshape(-1))
        if w.size != self.N:
            raise OdefError(f"log_weights: {w.size} values for {self.N} trajectories")
        # Every shard is bound to its new block before the old blocks are let go (no context is left pointing at freed
        # memory if an upload or a bind raises), and only then are the passes run.
        bufs = [_to_device((w[lo:lo + count],), self._devices[g])[0] for g, (lo, count) in enumerate(map(self.shard, range(self.G)))]
        old = getattr(self, "_log_weight_bufs", None)
        self._log_weight_bufs = [old, bufs]  # device memory owned by torch, kept alive by the group
        for g, buf in enumerate(bufs):
            c = self.lib.odef_group_ctx(self._h, g)
            if self.lib.odef_bind_device(c, W_LOGWEIGHT, _vp(buf.data_ptr()), buf.numel() * 8) != 0:
                raise OdefError(self.lib.odef_last_error(c).decode())
        self._log_weight_bufs = bufs
        parts = []
        for g in range(self.G):
            c = self.lib.odef_group_ctx(self._h, g)
            parts.append(tuple(_fetch(self.lib, c, f).reshape(_DERIVED[f][1](self))
                               for f in (wsummary_field(source, qty) for qty in range(6))))
        return merge_weighted_moments(parts)

    def ensemble_quantiles(self, source: int, probs=None):
        """Refused: the quantiles of the shards do not pool (exact pooling would all-reduce the per-pass histograms)."""
        raise OdefError("ensemble_quantiles of a sharded ensemble: the quantiles of the shards do not pool into those of the "
                        "whole ensemble; solve the ensemble on one device (Context.ensemble_quantiles)")

    def shard_kernel_ms(self, which=0):
        ms = []
        for g in range(self.G):
            t, n = C.c_float(), C.c_int()
            self.lib.odef_kernel_time_ms(self.lib.odef_group_ctx(self._h, g), which, C.byref(t), C.byref(n))
            ms.append(float(t.value))
        return ms


def compile_rhs(name: str, source: str, d: int, n_params: int, struct_name: Optional[str] = None) -> str:
    """Register a user vector field from HIP C++ source (`odef_rhs_compile`, include/odefilter.h): the stand-in for the
    closure `f` (+ `jac`) the reference calls at src/perform_step.jl:106,116-121.  `source` defines a struct
    `struct_name` (default: `name`) with the interface of csrc/rhs.h.  Afterwards `name` can be used wherever a
    compiled-in vector field name is accepted (`ODEProblem(name, ...)`, `Context(name, ...)`).  Raises OdefError with
    the compiler log when the text does not compile.

    A time-dependent field f(u, p, t) sets `static constexpr bool has_time = true;` and takes the absolute time behind
    `p`: `f(const T (&u)[d], const double* p, T t, T (&du)[d])`, `jac(u, p, double t, J)` (optional), and `analytic(u0, p,
    t0, t, out)` (optional).  The step evaluates it at its new time, the Taylor initialisation differentiates in t too;
    `solve` takes no new keyword.  It runs on the lane and row-team kernels (d <= 10, d (q + 1) <= 20): above, creating
    the context raises OdefError."""
    lib = load_library()
    rid = C.c_int32(-1)
    inc = os.path.join(_HERE, "csrc").encode()
    rc = lib.odef_rhs_compile((struct_name or name).encode(), source.encode(), int(d), int(n_params), inc, C.byref(rid))
    if rc != 0:
        raise OdefError(lib.odef_last_error(None).decode())
    RHS[name] = int(rid.value)
    RHS_DIMS[name] = (int(d), int(n_params))
    return name


def _as_dp(a: np.ndarray):
    return a.ctypes.data_as(_dp)


class Context:
    """RAII wrapper of `odef_ctx` (the device-side `GaussianODEFilterCache`, src/caches.jl:5-40)."""

    def __init__(self, rhs: str, order: int, alg: int, n_traj: int, *, diffusion="dynamic", smooth=False,
                 save_everystep=True, params_shared=True, device=-1, want_loglik=True):
        self.lib = load_library()
        if rhs not in RHS:
            raise OdefError(f"unknown vector field {rhs!r}; the device registry has {sorted(RHS)}")
        d, npar = RHS_DIMS[rhs]
        cfg = OdefConfig()
        cfg.struct_size = C.sizeof(OdefConfig)
        cfg.alg, cfg.order, cfg.diffusion = alg, order, DIFFUSION[diffusion]
        cfg.smooth, cfg.rhs_id, cfg.d, cfg.n_params = int(smooth), RHS[rhs], d, npar
        cfg.params_shared = int(params_shared)
        cfg.save_mode = SAVE_EVERYSTEP if (save_everystep or smooth) else SAVE_FINAL
        cfg.device, cfg.want_loglik, cfg.n_traj = device, int(want_loglik), n_traj
        self.cfg = cfg
        self.mv = diffusion in MV_DIFFUSIONS
        self.d, self.q, self.N = d, order, n_traj
        self.D = d * (order + 1)
        self.TRI = self.D * (self.D + 1) // 2
        h = _vp()
        rc = self.lib.odef_create(C.byref(h), C.byref(cfg))
        if rc != 0:
            raise OdefError(self.lib.odef_last_error(None).decode())
        self._h = h

    def _chk(self, rc):
        if rc != 0:
            raise OdefError(self.lib.odef_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self.lib.odef_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_stream(self, stream_ptr: int):
        self._chk(self.lib.odef_set_stream(self._h, _vp(stream_ptr)))

    def set_problem(self, u0: np.ndarray, p: Optional[np.ndarray], t0: float):
        u0 = np.ascontiguousarray(u0, dtype=np.float64)
        if u0.shape != (self.N, self.d):
            raise OdefError(f"u0 must have shape ({self.N}, {self.d}), got {u0.shape}")
        pp = None
        if self.cfg.n_params > 0:
            p = np.ascontiguousarray(p, dtype=np.float64)
            want = (self.cfg.n_params,) if self.cfg.params_shared else (self.N, self.cfg.n_params)
            if p.shape != want:
                raise OdefError(f"p must have shape {want}, got {p.shape}")
            pp = _as_dp(p)
        self._chk(self.lib.odef_set_problem(self._h, _as_dp(u0), pp, float(t0)))

    def set_problem_device(self, d_u0_ptr: int, d_p_ptr: int, t0: float):
        self._chk(self.lib.odef_set_problem_device(self._h, _vp(d_u0_ptr), _vp(d_p_ptr), float(t0)))

    def set_problem_perturbed(self, base_u0, p, t0, scale, seed=0x0DEF17E5, first_index=0, n_perturbed=None):
        base = np.ascontiguousarray(base_u0, dtype=np.float64)
        pp = _as_dp(np.ascontiguousarray(p, dtype=np.float64)) if self.cfg.n_params > 0 else None
        npert = self.d if n_perturbed is None else n_perturbed
        self._chk(self.lib.odef_set_problem_perturbed(self._h, _as_dp(base), pp, float(t0), float(scale),
                                                      C.c_uint64(seed), C.c_int64(first_index), npert))

    def solve_fixed(self, tgrid: Sequence[float]):
        tg = np.ascontiguousarray(tgrid, dtype=np.float64)
        self._chk(self.lib.odef_solve_fixed(self._h, _as_dp(tg), len(tg)))

    def solve_adaptive(self, t1, abstol=1e-6, reltol=1e-3, dt0=1e-3, controller: Optional[OdefController] = None,
                       max_steps=4096):
        cp = C.byref(controller) if controller is not None else None
        self._chk(self.lib.odef_solve_adaptive(self._h, float(t1), float(abstol), float(reltol), float(dt0), cp,
                                               int(max_steps)))

    def smooth(self):
        self._chk(self.lib.odef_smooth(self._h))

    def dense_output(self, tq, smoothed: bool):
        """Posterior at the times `tq` for every trajectory: (mean [n_q, D, N], cov_tril [n_q, TRI, N])."""
        tq = np.ascontiguousarray(tq, dtype=np.float64)
        self._chk(self.lib.odef_dense_output(self._h, _as_dp(tq), len(tq), int(smoothed)))
        m, c = _fetch(self.lib, self._h, F_DENSE_MEAN), _fetch(self.lib, self._h, F_DENSE_COV_TRIL)
        return m.reshape(len(tq), self.D, self.N), c.reshape(len(tq), self.TRI, self.N)

    def sample_states(self, n: int, seed: int, noise_scale: float = 1.0):
        """n joint posterior draws of the state path per trajectory: [n_save, D, n, N]."""
        self._chk(self.lib.odef_sample(self._h, int(n), int(seed) & 0xFFFFFFFFFFFFFFFF, float(noise_scale)))
        return _fetch(self.lib, self._h, F_SAMPLES).reshape(self.n_save, self.D, int(n), self.N)

    def dense_sample_states(self, tq, n: int, seed: int, noise_scale: float = 1.0):
        """n joint draws of the state path on the times tq (filter-interpolated states): [n_q, D, n, N]."""
        tq = np.ascontiguousarray(tq, float)
        self._chk(self.lib.odef_dense_sample(self._h, tq.ctypes.data_as(C.POINTER(C.c_double)), len(tq), int(n),
                                             int(seed) & 0xFFFFFFFFFFFFFFFF, float(noise_scale)))
        return _fetch(self.lib, self._h, F_SAMPLES).reshape(len(tq), self.D, int(n), self.N)

    def synchronize(self):
        self._chk(self.lib.odef_synchronize(self._h))

    @property
    def n_save(self) -> int:
        return int(self.lib.odef_n_save(self._h))

    def field_bytes(self, f: int) -> int:
        b = C.c_size_t()
        self._chk(self.lib.odef_field_bytes(self._h, f, C.byref(b)))
        return b.value

    def get(self, f: int) -> np.ndarray:
        """Field in the device layout (include/odefilter.h), as a flat numpy array reshaped."""
        out = _fetch(self.lib, self._h, f)
        if f in _DERIVED:
            return out.reshape(_DERIVED[f][1](self))
        ns, N = self.n_save, self.N
        if f in (F_MEAN, F_SMOOTH_MEAN):
            return out.reshape(ns, self.D, N)
        if f in (F_COV_TRIL, F_SMOOTH_COV_TRIL):
            return out.reshape(ns, self.TRI, N)
        if f == F_DIFFUSION:
            return out.reshape(ns, self.d, N) if self.mv else out.reshape(ns, N)
        if f == F_T:
            return out.reshape(ns, N) if out.size == ns * N and out.size != ns else out
        if f == F_U0:
            return out.reshape(self.d, N)
        if f == F_LINEARIZE_AT:
            return out.reshape(-1, self.d, N)
        return out

    def ensemble_moments(self, source: int):
        """Ensemble summary per time of the filter (0), smoothed (1) or last dense-output (2) records, reduced on the device
        (`odef_summary_field`): (count [n_t] int64, mean [n_t, d], within [n_t, tri], between [n_t, tri]), tri = d(d+1)/2 packed
        lower triangles.  The first request after the records changed launches the reduction; later ones read the cache."""
        return tuple(self.get(summary_field(source, qty)) for qty in range(4))

    def bind_quantile_probs(self, ptr: int, P: int):
        """The probabilities of `ensemble_quantiles`: double [P] in device memory that stays the caller's (read only),
        1 <= P <= 8, each in [0, 1]; they need not be sorted or distinct.  ptr = 0 lets them go."""
        self._quantile_probs = None  # what is bound now is the caller's
        self._chk(self.lib.odef_bind_device(self._h, Q_PROBS, _vp(ptr) if ptr else None, int(P) * 8))

    def ensemble_quantiles(self, source: int, probs=None):
        """Type-7 quantiles (numpy's default, Julia's `quantile`) of every solution component of the posterior means over the
        included trajectories, per time of the filter (0), smoothed (1) or last dense-output (2) records, selected on the device
        (`odef_quantile_field`): (count [n_t] int64, q [n_t, P, d]).  `probs`: uploaded and bound first, unless they are bit for bit
        those this method bound last (a bind drops the cache); None: those bound already.  Exact: q is the order statistic itself, interpolated with one rounding per operation.  The
        first request after the records or the probabilities changed launches the pass; later ones read the cache."""
        if probs is not None:
            p = np.ascontiguousarray(np.atleast_1d(np.asarray(probs, float)).reshape(-1))
            if getattr(self, "_quantile_probs", None) != p.tobytes():
                # device memory owned by torch, kept alive by the context
                self._quantile_bufs = _to_device((p,), self.cfg.device) if p.size else None
                self.bind_quantile_probs(self._quantile_bufs[0].data_ptr() if p.size else 0, p.size)
                self._quantile_probs = p.tobytes() if p.size else None
        return self.get(quantile_field(source, Q_COUNT)), self.get(quantile_field(source, Q_QUANTILES))

    def bind_log_weights(self, ptr: int, N: int):
        """The unnormalised log-weights of `weighted_moments`: double [N] in device memory that stays the caller's (read only,
        never written); N is the context's number of trajectories.  A value that is not finite excludes its trajectory.  ptr = 0
        lets them go."""
        self._log_weights = None  # what is bound now is the caller's
        self._chk(self.lib.odef_bind_device(self._h, W_LOGWEIGHT, _vp(ptr) if ptr else None, int(N) * 8))

    def _bind_log_weight_tensor(self, tensor, key):
        """Binds a float64 [N] torch tensor on the context's device and keeps it alive; `key`: its bytes when they are known on
        the host (a later request with the same bytes binds nothing), else None."""
        if tensor.numel() != self.N:
            raise OdefError(f"log_weights: {tensor.numel()} values for {self.N} trajectories")
        self._log_weight_buf = tensor
        self.bind_log_weights(tensor.data_ptr(), self.N)
        self._log_weights = key

    def weighted_moments(self, source: int, log_weights=None):
        """Weighted ensemble summary per time of the filter (0), smoothed (1) or last dense-output (2) records, reduced on the
        device (`odef_wsummary_field`): (count [n_t] int64, mean [n_t, d], within [n_t, tri], between [n_t, tri], log_evidence
        [n_t], ess [n_t]) of the mixture with weights proportional to exp(log_weights).  `log_weights` [N] (a numpy array, or a
        torch tensor on any device, which is copied to the host for the comparison -- 8 N bytes -- and uploaded like an array; weights
        that must not leave the device are bound with `bind_log_weights`): uploaded and bound first, unless they are bit for bit those this method bound last (a bind drops the
        cache); None: those bound already.  The first request after the records or the weights changed launches the pass; later
        ones read the cache."""
        if log_weights is not None:
            if hasattr(log_weights, "detach"):  # a torch tensor
                log_weights = log_weights.detach().cpu().numpy()
            w = np.ascontiguousarray(np.asarray(log_weights, float).reshape(-1))
            if w.size != self.N:
                raise OdefError(f"log_weights: {w.size} values for {self.N} trajectories")
            if getattr(self, "_log_weights", None) != w.tobytes():
                # device memory owned by torch, kept alive by the context
                self._bind_log_weight_tensor(_to_device((w,), self.cfg.device)[0], w.tobytes())
        return tuple(self.get(wsummary_field(source, qty)) for qty in range(6))

    def bind_data_loglik_as_weights(self, log_prior=None):
        """Binds log-weights = the data log-likelihood of the bound observations (`ODEF_L_DATA_LOGLIK`, computed if need be)
        + `log_prior` [N] if given, without a trip through the host: a device-to-device COPY into a tensor the context owns
        (the likelihood's own cache is freed when it is dropped, so its pointer is never bound)."""
        import torch

        ptr, nbytes = self.device_ptr(L_DATA_LOGLIK)

        class Raw:
            __cuda_array_interface__ = {"shape": (nbytes // 8,), "typestr": "<f8", "data": (ptr, False), "version": 2}

        dev = torch.device("cuda", int(self.cfg.device) if self.cfg.device >= 0 else torch.cuda.current_device())
        w = torch.as_tensor(Raw(), device=dev).clone()
        if log_prior is not None:
            lp = np.ascontiguousarray(np.asarray(log_prior, float).reshape(-1))
            if lp.size != self.N:
                raise OdefError(f"log_prior: {lp.size} values for {self.N} trajectories")
            w += torch.from_numpy(lp).to(dev)
        torch.cuda.synchronize(dev)
        self._bind_log_weight_tensor(w, None)

    @staticmethod
    def _solution_errors(lib, h, source: int):
        return {key: _fetch(lib, h, errors_field(source, qty))
                for key, qty in (("l∞", E_LINF), ("l2", E_L2), ("final", E_FINAL), ("chi2", E_CHI2), ("nused", E_NUSED))}

    def solution_errors(self, source: int):
        """Per-trajectory errors of the filter (0) or smoothed (1) solution against the truth -- the vector field's `analytic`, or
        a reference bound with `bind_reference` --, reduced on the device (`odef_errors_field`): dict with "l∞", "l2", "final"
        (DiffEqBase's sol.errors), "chi2" (mean_k e' Sigma^+ e / d, ~ 1 for a calibrated posterior), each [N], and "nused"."""
        return self._solution_errors(self.lib, self._h, source)

    def bind_reference(self, ptr: int, nbytes: int):
        """The truth of `solution_errors` for a field without a closed form (`appxtrue`): [n_save][d][N] doubles in device memory,
        read only -- e.g. a tight solve's `odef_dense_output` on this grid.  Fixed grids only; ptr = 0 lets it go."""
        self._chk(self.lib.odef_bind_device(self._h, E_REFERENCE, _vp(ptr) if ptr else None, nbytes))

    def bind_observations(self, save_ptr: int, comp_ptr: int, value_ptr: int, noise_ptr: int, M: int, o: int, per_trajectory: bool):
        """The observations of `data_loglik`, device memory that stays the caller's (read only): save indices int64 [M],
        components int64 [o], values double [M][o] (shared) or [M][o][N] (per trajectory), noise variances double [o]."""
        nv = M * o * (self.N if per_trajectory else 1) * 8
        for f, ptr, nb in ((L_OBS_TIME, 0, 0), (L_OBS_SAVE, save_ptr, M * 8), (L_OBS_COMPONENT, comp_ptr, o * 8),
                           (L_OBS_VALUE, value_ptr, nv), (L_OBS_NOISE, noise_ptr, o * 8)):
            self._chk(self.lib.odef_bind_device(self._h, f, _vp(ptr) if ptr else None, nb))

    def bind_observation_times(self, time_ptr: int, comp_ptr: int, value_ptr: int, noise_ptr: int, M: int, o: int,
                               per_trajectory: bool):
        """The observations of `data_loglik` given by TIME, after a fixed-grid or an adaptive solve: times double [M], strictly
        increasing from t0 on (they need not be save times); the other three as in `bind_observations`.  Unbinds the save
        indices: the two ways of saying where the observations lie exclude each other."""
        nv = M * o * (self.N if per_trajectory else 1) * 8
        for f, ptr, nb in ((L_OBS_SAVE, 0, 0), (L_OBS_TIME, time_ptr, M * 8), (L_OBS_COMPONENT, comp_ptr, o * 8),
                           (L_OBS_VALUE, value_ptr, nv), (L_OBS_NOISE, noise_ptr, o * 8)):
            self._chk(self.lib.odef_bind_device(self._h, f, _vp(ptr) if ptr else None, nb))

    @staticmethod
    def _data_loglik(lib, h, bufs=None, by_time=False):
        """(loglik [N], mahalanobis [N]) of the context `h`; `bufs`: torch tensors (saves or -- `by_time` -- times, comps, values,
        noise) to bind first; the other of OBS_SAVE / OBS_TIME is unbound."""
        if bufs is not None:
            first, other = (L_OBS_TIME, L_OBS_SAVE) if by_time else (L_OBS_SAVE, L_OBS_TIME)
            if lib.odef_bind_device(h, other, None, 0) != 0:
                raise OdefError(lib.odef_last_error(h).decode())
            for f, b in zip((first, L_OBS_COMPONENT, L_OBS_VALUE, L_OBS_NOISE), bufs):
                if lib.odef_bind_device(h, f, _vp(b.data_ptr()), b.numel() * 8) != 0:
                    raise OdefError(lib.odef_last_error(h).decode())
        return tuple(_fetch(lib, h, f) for f in (L_DATA_LOGLIK, L_DATA_MAHALANOBIS))

    def data_loglik(self):
        """Per-trajectory log-likelihood of the bound observations under the posterior of the last solve (by save index: fixed
        grids; by time, `bind_observation_times`: fixed and adaptive), and the
        Mahalanobis sum (chi^2 with M o degrees of freedom for a calibrated model), reduced on the device (`odef_data_field`):
        (loglik [N], mahalanobis [N]).  The first request after the records or the observations changed launches the pass."""
        return self._data_loglik(self.lib, self._h)

    def bind_event(self, spec_ptr: int, level_ptr: int, per_trajectory: bool):
        """The inputs of `events`, device memory that stays the caller's (read only): spec int64 [3] {component, direction, K}
        and the level, one double or -- `per_trajectory` -- [N]."""
        for f, ptr, nb in ((EV_SPEC, spec_ptr, 24), (EV_LEVEL, level_ptr, 8 * (self.N if per_trajectory else 1))):
            self._chk(self.lib.odef_bind_device(self._h, f, _vp(ptr) if ptr else None, nb))

    @staticmethod
    def _events(lib, h, shape, source: int, bufs=None) -> "Events":
        """`Events` of the context `h` (`shape`: anything with d and N of that context's family; the arrays are reshaped by their
        own trajectory count); `bufs`: torch tensors (spec, level) to bind first."""
        if bufs is not None:
            for f, b in zip((EV_SPEC, EV_LEVEL), bufs):
                if lib.odef_bind_device(h, f, _vp(b.data_ptr()), b.numel() * 8) != 0:
                    raise OdefError(lib.odef_last_error(h).decode())
        count = _fetch(lib, h, event_field(source, EV_COUNT))
        n, d = count.size, shape.d
        arr = [count]
        for qty in range(1, 7):
            a = _fetch(lib, h, event_field(source, qty))
            arr.append(a.reshape(-1, d, n) if qty == EV_U else a.reshape(-1, n))
        return Events.from_abi(arr)

    def events(self, source: int) -> "Events":
        """Level crossings per trajectory for the bound spec and level (`bind_event`) on the filter (0) or smoothed (1) posterior,
        located on the device (`odef_event_field`).  The first request after the records or an input changed launches the pass
        (a scan of one row of the mean records, then bracketed Newton on the dense posterior); later ones read the cache."""
        return self._events(self.lib, self._h, self, source)

    def device_ptr(self, f: int):
        p, b = _vp(), C.c_size_t()
        self._chk(self.lib.odef_get_device(self._h, f, C.byref(p), C.byref(b)))
        return p.value, b.value

    def bind_device(self, f: int, ptr: int, nbytes: int):
        self._chk(self.lib.odef_bind_device(self._h, f, _vp(ptr), nbytes))

    def kernel_name(self, which=0) -> str:
        """Name of the kernel the last filter (0) / smoother (1) / ensemble-summary (2) / solution-error (3) / data-likelihood
        (4) / event-location (5) / ensemble-quantile (6) / weighted-summary (7) pass launched, as a profiler prints it."""
        buf = C.create_string_buffer(256)
        self._chk(self.lib.odef_kernel_name(self._h, which, buf, 256))
        return buf.value.decode()

    def kernel_time_ms(self, which=0):
        ms, n = C.c_float(), C.c_int()
        self._chk(self.lib.odef_kernel_time_ms(self._h, which, C.byref(ms), C.byref(n)))
        return ms.value, n.value


# ---- constants and step-level functions --------------------------------------------------


def ibm(d: int, q: int):
    """`ProbNumDiffEq.ibm(d, q)` (src/priors.jl:7-59): A (upper triangular), Q_L = chol(Q).L."""
    lib = load_library()
    D = d * (q + 1)
    A, QL = np.zeros((D, D)), np.zeros((D, D))
    if lib.odef_ibm(d, q, _as_dp(A), _as_dp(QL)) != 0:
        raise OdefError("odef_ibm failed")
    return A, QL


def preconditioner(d: int, q: int):
    """`ProbNumDiffEq.preconditioner(T, d, q)` (src/preconditioning.jl:1-17): returns P(h) -> diag."""
    lib = load_library()

    def P(h: float) -> np.ndarray:
        out = np.zeros(d * (q + 1))
        if lib.odef_preconditioner(d, q, float(h), _as_dp(out)) != 0:
            raise OdefError("odef_preconditioner failed")
        return out

    return P


def _batched(mu, L):
    mu = np.ascontiguousarray(np.atleast_2d(np.asarray(mu, float)))
    L = np.ascontiguousarray(np.asarray(L, float).reshape(mu.shape[0], mu.shape[1], mu.shape[1]))
    return mu, L


def predict(mu, L, A, Q_L):
    """`predict(x_curr, Ah, Qh)` (src/filtering.jl:56) on a batch; returns (mean, cov)."""
    lib = load_library()
    mu, L = _batched(mu, L)
    n, D = mu.shape
    A = np.ascontiguousarray(A, float); Q_L = np.ascontiguousarray(Q_L, float)
    mo, co = np.empty((n, D)), np.empty((n, D, D))
    if lib.odef_predict(D, n, _as_dp(mu), _as_dp(L), _as_dp(A), _as_dp(Q_L), _as_dp(mo), _as_dp(co)) != 0:
        raise OdefError("odef_predict failed")
    return mo, co


def update(mu_pred, L_pred, H, z):
    """`update(x_pred, measurement, H, R=0)` (src/filtering.jl:97) on a batch; returns (mean, cov)."""
    lib = load_library()
    mu, L = _batched(mu_pred, L_pred)
    n, D = mu.shape
    H = np.ascontiguousarray(np.asarray(H, float).reshape(n, -1, D))
    o = H.shape[1]
    z = np.ascontiguousarray(np.asarray(z, float).reshape(n, o))
    mo, co = np.empty((n, D)), np.empty((n, D, D))
    if lib.odef_update(D, o, n, _as_dp(mu), _as_dp(L), _as_dp(H), _as_dp(z), _as_dp(mo), _as_dp(co)) != 0:
        raise OdefError("odef_update failed")
    return mo, co


def smooth_step(mu, L, mu_s, L_s, A, Q_L):
    """`smooth(x_curr, x_next_smoothed, Ah, Qh)` (src/filtering.jl:136) on a batch; returns (mean, cov)."""
    lib = load_library()
    mu, L = _batched(mu, L)
    mu_s, L_s = _batched(mu_s, L_s)
    n, D = mu.shape
    A = np.ascontiguousarray(A, float); Q_L = np.ascontiguousarray(Q_L, float)
    mo, co = np.empty((n, D)), np.empty((n, D, D))
    if lib.odef_smooth_step(D, n, _as_dp(mu), _as_dp(L), _as_dp(mu_s), _as_dp(L_s), _as_dp(A), _as_dp(Q_L),
                            _as_dp(mo), _as_dp(co)) != 0:
        raise OdefError("odef_smooth_step failed")
    return mo, co


# ---- the solver interface (names of src/algorithms.jl and DiffEqBase) ---------------------


@dataclass(frozen=True)
class EK0:
    """`EK0(; prior=:ibm, order=3, diffusionmodel=:dynamic, smooth=true)` (src/algorithms.jl:23-28)."""
    prior: str = "ibm"
    order: int = 3
    diffusionmodel: str = "dynamic"
    smooth: bool = True
    _id = EK0_ID


@dataclass(frozen=True)
class EK1:
    """`EK1(; prior=:ibm, order=3, diffusionmodel=:dynamic, smooth=true)` (src/algorithms.jl:46-51)."""
    prior: str = "ibm"
    order: int = 3
    diffusionmodel: str = "dynamic"
    smooth: bool = True
    _id = EK1_ID


class IEKS:
    """`IEKS(; prior=:ibm, order=1, diffusionmodel=:dynamic, linearize_at=nothing)` (src/ieks.jl:2-41): the iterated extended
    Kalman smoother of Tronarp et al.  `smooth` is always true.  `linearize_at`: a previous IEKS or EK1 `EnsembleSolution`
    (smoothed, same prior, order and diffusion model, same ensemble size) whose smoothed u the Jacobians of a plain
    `solve(prob, IEKS(linearize_at=sol), ...)` are evaluated at; `solve_ieks` ignores it and starts from EK1, as the
    reference's loop does."""
    _id = IEKS_ID
    smooth = True

    def __init__(self, prior: str = "ibm", order: int = 1, diffusionmodel: str = "dynamic", linearize_at=None):
        if linearize_at is not None:  # src/ieks.jl:32-38
            if not isinstance(linearize_at, EnsembleSolution):
                raise AssertionError("linearize_at must be a solution (EnsembleSolution)")
            la = linearize_at.alg
            if la.prior != prior:
                raise AssertionError(f"linearize_at was solved with prior {la.prior!r}, not {prior!r}")
            if la.order != order:
                raise AssertionError(f"linearize_at was solved with order {la.order}, not {order}")
            if la.diffusionmodel != diffusionmodel:
                raise AssertionError(f"linearize_at was solved with diffusionmodel {la.diffusionmodel!r}, not {diffusionmodel!r}")
            if not la.smooth:
                raise AssertionError("linearize_at must be a smoothed solution (smooth=true)")
        self.prior, self.order, self.diffusionmodel, self.linearize_at = prior, order, diffusionmodel, linearize_at

    def __repr__(self):
        return (f"IEKS(prior={self.prior!r}, order={self.order}, diffusionmodel={self.diffusionmodel!r}, "
                f"linearize_at={'None' if self.linearize_at is None else 'EnsembleSolution'})")


@dataclass
class ODEProblem:
    """`ODEProblem(f, u0, tspan, p)`.  `f` names a vector field of the device registry
    (a GPU kernel cannot call a host closure)."""
    f: str
    u0: Sequence[float]
    tspan: tuple
    p: Sequence[float] = ()

    def __post_init__(self):
        if np.ndim(self.u0) != 1:
            # src/caches.jl:46-49, test/errors.jl:11-14
            raise OdefError("Problems which are not scalar- or vector-valued (e.g. u0 is a scalar or a matrix) "
                            "are currently not supported")


@dataclass
class EnsembleProblem:
    """`EnsembleProblem(prob; prob_func)`: either explicit initial values `u0s[N, d]` (and
    optionally `ps[N, n_params]`), or the synthetic perturbation of SURVEY.md 8(d) generated
    on the device: u0_i = u0 + scale*(2U-1), U from splitmix64(seed + ...)."""
    prob: ODEProblem
    u0s: Optional[np.ndarray] = None
    ps: Optional[np.ndarray] = None
    perturb_scale: Optional[float] = None
    seed: int = 0x0DEF17E5
    first_index: int = 0
    n_perturbed: Optional[int] = None


@dataclass(frozen=True)
class EnsembleHIP:
    """Ensemble algorithm: all trajectories on one MI355X (`device`), one lane per trajectory.

    `distributed=True` (one process per GPU under torchrun): every rank solves the contiguous block of the trajectory
    index `dist.shard_bounds` assigns to it on the GPU `LOCAL_RANK`, nothing is exchanged while stepping, and
    `EnsembleSolution.gather_final()` is the single RCCL all-gather of the path."""
    device: int = -1
    distributed: bool = False
    backend: str = "nccl"  # torch.distributed backend of the distributed path ("nccl" = RCCL over xGMI; "gloo" for CPU tests)


def shard_ensemble(prob: "EnsembleProblem", trajectories: Optional[int], rank: int, world: int):
    """(per-rank EnsembleProblem, n_local, (lo, hi)): contiguous block of the trajectory index.  The synthetic ensemble
    keeps its GLOBAL numbering (first_index + lo), explicit u0s / ps are sliced -- so the union of the shards is exactly
    the ensemble one larger solve would produce."""
    from . import dist as od

    total = len(prob.u0s) if prob.u0s is not None else trajectories
    if total is None:
        raise OdefError("trajectories is required")
    lo, hi = od.shard_bounds(int(total), rank, world)
    if prob.u0s is not None:
        local = EnsembleProblem(prob.prob, u0s=np.asarray(prob.u0s)[lo:hi], ps=None if prob.ps is None else np.asarray(prob.ps)[lo:hi])
    else:
        local = EnsembleProblem(prob.prob, ps=None if prob.ps is None else np.asarray(prob.ps)[lo:hi],
                                perturb_scale=prob.perturb_scale, seed=prob.seed, first_index=prob.first_index + lo,
                                n_perturbed=prob.n_perturbed)
    return local, hi - lo, (lo, hi)


def fixed_time_grid(t0: float, t1: float, dt: float, tstops: Optional[Sequence[float]] = None) -> np.ndarray:
    """OrdinaryDiffEq's fixed-step grid: t += dt, every step clipped onto the next tstop (the end of the time span is
    one), with the 100-eps snap of the integrator loop."""
    if not (np.isfinite(dt) and dt > 0.0):
        raise OdefError(f"dt must be positive and finite, got {dt!r}")
    if not (t1 > t0):
        raise OdefError(f"tspan must be increasing, got ({t0!r}, {t1!r})")
    stops = sorted({float(x) for x in (tstops if tstops is not None else []) if t0 < float(x) < t1} | {float(t1)})
    ts = [t0]
    t = t0
    eps = np.finfo(float).eps
    for stop in stops:
        while t < stop:
            h = min(dt, stop - t)
            tn = t + h
            if abs(tn - stop) < 100 * eps * max(abs(tn), abs(stop)):
                tn = stop
            ts.append(tn)
            t = tn
    return np.array(ts)


def unpack_tril(c: np.ndarray, D: int) -> np.ndarray:
    """[..., TRI] -> [..., D, D] symmetric."""
    out = np.empty(c.shape[:-1] + (D, D))
    il = np.tril_indices(D)
    out[..., il[0], il[1]] = c
    out[..., il[1], il[0]] = c
    return out


def merge_moments(parts):
    """Exact pooled combination of per-shard ensemble summaries.  parts: iterable of (n [n_t], mean [n_t, d], within [n_t, tri],
    between [n_t, tri]); shards with n = 0 at a time are skipped there.  n = sum n_r, mean = sum n_r mean_r / n, W = sum n_r W_r / n,
    B = sum n_r (B_r + (mean_r - mean)(mean_r - mean)') / n; with n = 0 the moments are NaN.  Pure numpy."""
    parts = [(np.asarray(n, np.int64), np.asarray(m, float), np.asarray(w, float), np.asarray(b, float)) for n, m, w, b in parts]
    if not parts:
        raise OdefError("merge_moments: no parts")
    n_t, d = parts[0][1].shape
    il = np.tril_indices(d)
    n = sum(p[0] for p in parts)
    nn = np.where(n > 0, n, 1).astype(float)[:, None]
    wgt = [(p[0] / nn[:, 0])[:, None] for p in parts]  # n_r / n
    mean = sum(np.where(p[0][:, None] > 0, w_r * p[1], 0.0) for p, w_r in zip(parts, wgt))
    within = sum(np.where(p[0][:, None] > 0, w_r * p[2], 0.0) for p, w_r in zip(parts, wgt))
    between = np.zeros_like(within)
    for p, w_r in zip(parts, wgt):
        dm = np.where(p[0][:, None] > 0, p[1] - mean, 0.0)
        between += np.where(p[0][:, None] > 0, w_r * (p[3] + dm[:, il[0]] * dm[:, il[1]]), 0.0)
    empty = (n == 0)[:, None]
    return n, np.where(empty, np.nan, mean), np.where(empty, np.nan, within), np.where(empty, np.nan, between)


def merge_weighted_moments(parts):
    """Pooled combination of per-shard weighted ensemble summaries.  parts: iterable of (n [n_t], mean [n_t, d], within [n_t, tri],
    between [n_t, tri], log_evidence [n_t], ess [n_t]), every shard with its own shift L_r.  The absolute mass of shard r at a
    time is n_r exp(log_evidence_r) = sum_i exp(l_i); the masses are combined by log-sum-exp, omega_r = mass_r / sum mass, and
    the moments pool as in `merge_moments` with omega_r in place of n_r / n.  sum v^2 of a shard is recovered as mass_r^2 / ess_r,
    so ESS = 1 / sum_r omega_r^2 / ess_r; log_evidence = log sum mass - log n with n = sum n_r.  A shard without mass at a time (n_r
    = 0, or every weight underflowed) is skipped there; with n = 0 everything is NaN, with n > 0 and no mass the moments and ESS are
    NaN and log_evidence is -inf, as on one device.  Pure numpy."""
    parts = [(np.asarray(p[0], np.int64),) + tuple(np.asarray(a, float) for a in p[1:]) for p in parts]
    if not parts:
        raise OdefError("merge_weighted_moments: no parts")
    for p in parts:
        if len(p) != 6:
            raise OdefError("merge_weighted_moments: a part is (count, mean, within, between, log_evidence, ess)")
    n_t, d = parts[0][1].shape
    il = np.tril_indices(d)
    n = sum(p[0] for p in parts)
    with np.errstate(divide="ignore", invalid="ignore"):
        logm = [np.where(p[0] > 0, np.log(np.maximum(p[0], 1).astype(float)) + p[4], -np.inf) for p in parts]  # log mass_r
        top = np.max(logm, axis=0)
        has_mass = np.isfinite(top)
        shift = np.where(has_mass, top, 0.0)
        rel = [np.where(np.isfinite(a), np.exp(a - shift), 0.0) for a in logm]
        total = sum(rel)
        omega = [np.where(has_mass, r / np.where(has_mass, total, 1.0), 0.0) for r in rel]
        log_evidence = np.where(has_mass, shift + np.log(np.where(has_mass, total, 1.0)), -np.inf) - np.log(n.astype(float))
        inv_ess = sum(np.where(o > 0, o * o / np.where(o > 0, p[5], 1.0), 0.0) for p, o in zip(parts, omega))
        ess = 1.0 / inv_ess
    live = [(o > 0)[:, None] for o in omega]
    mean = sum(np.where(l, o[:, None] * p[1], 0.0) for p, o, l in zip(parts, omega, live))
    within = sum(np.where(l, o[:, None] * p[2], 0.0) for p, o, l in zip(parts, omega, live))
    between = np.zeros_like(within)
    for p, o, l in zip(parts, omega, live):
        dm = np.where(l, p[1] - mean, 0.0)
        between += np.where(l, o[:, None] * (p[3] + dm[:, il[0]] * dm[:, il[1]]), 0.0)
    dead = ~has_mass
    nan = lambda a: np.where(dead[:, None], np.nan, a)  # noqa: E731
    return (n, nan(mean), nan(within), nan(between), np.where(n == 0, np.nan, log_evidence), np.where(dead, np.nan, ess))


@dataclass
class EnsembleSummary:
    """Per-time summary of an ensemble: the equal-weight mixture of the trajectories' Gaussian posteriors has mean `mean` and
    covariance `cov` = `cov_within` (mean posterior covariance) + `cov_between` (covariance of the posterior means, divisor n).
    `n` counts the trajectories included at each time (Success retcode, finite mean); with n = 0 the moments are NaN."""
    t: np.ndarray            # [n_t]
    n: np.ndarray            # [n_t] int64
    mean: np.ndarray         # [n_t, d]
    cov_within: np.ndarray   # [n_t, d, d]
    cov_between: np.ndarray  # [n_t, d, d]
    # the order statistics of the posterior means, with `sol.summary(quantiles=(lo, hi))` (SciML's EnsembleSummary names)
    med: Optional[np.ndarray] = None             # [n_t, d]
    qlow: Optional[np.ndarray] = None            # [n_t, d]
    qhigh: Optional[np.ndarray] = None           # [n_t, d]
    quantile_probs: Optional[tuple] = None       # (lo, hi)
    # with `sol.summary(log_weights=...)` / `sol.posterior_predictive(...)`: the mixture is weighted by w_i proportional to
    # exp(log_weights_i) instead of 1 / n, and these two say how far to trust it
    ess: Optional[np.ndarray] = None             # [n_t] effective sample size (sum w)^2 / sum w^2, in [1, n]
    log_evidence: Optional[np.ndarray] = None    # [n_t] log((1/n) sum_i exp log_weights_i)

    @classmethod
    def from_moments(cls, t, n, mean, within, between, log_evidence=None, ess=None):
        d = mean.shape[1]
        return cls(np.asarray(t, float).reshape(-1), n, mean, unpack_tril(within, d), unpack_tril(between, d),
                   ess=ess, log_evidence=log_evidence)

    @property
    def cov(self) -> np.ndarray:
        return self.cov_within + self.cov_between

    @property
    def std(self) -> np.ndarray:
        """[n_t, d]: square root of the diagonal of `cov`."""
        return np.sqrt(np.diagonal(self.cov, axis1=1, axis2=2))


@dataclass
class DEStats:
    nf: np.ndarray
    njacs: np.ndarray
    naccept: np.ndarray
    nreject: np.ndarray


class EnsembleSolution:
    """Per-trajectory `ProbODESolution` fields (src/solution.jl:8-24), batched.  Arrays are
    fetched from the device lazily and returned trajectory-major: mean[N, n_save, D]."""

    def __init__(self, ctx: Context, alg, adaptive: bool):
        self.ctx, self.alg, self.adaptive = ctx, alg, adaptive
        self.d, self.q, self.D = ctx.d, ctx.q, ctx.D
        self._cache = {}
        self.shard = None  # (lo, hi, total, world) of a distributed solve

    def final_mean(self) -> np.ndarray:
        """[N, D]: posterior mean of the state at each trajectory's last time (the filter state, which is also the
        smoothed one there, src/smoothing.jl:11)."""
        m = self._get(F_MEAN)  # [n_save, D, N]
        if not self.adaptive:
            return np.ascontiguousarray(m[-1].T)
        last = self._get(F_NSAVED).astype(np.int64) - 1
        return np.ascontiguousarray(m[last, :, np.arange(m.shape[2])])

    def gather_final(self) -> np.ndarray:
        """Distributed solves: the one collective of the path -- all-gather of the per-shard final means into
        [N_total, D] in global trajectory order on every rank (RCCL over xGMI; shards may differ by one row, so they
        are padded to the largest).  A non-distributed solve returns its own final means."""
        mine = self.final_mean()
        if self.shard is None or self.shard[3] == 1:
            return mine
        import torch

        from . import dist as od

        lo, hi, total, world = self.shard
        rows = -(-total // world)
        # the GPU this rank's context runs on (RCCL needs one distinct device per rank: never "the current device")
        dev = torch.device("cuda", int(self.ctx.cfg.device)) if torch.distributed.get_backend() == "nccl" else torch.device("cpu")
        buf = torch.zeros((rows, self.D), dtype=torch.float64, device=dev)
        buf[: hi - lo] = torch.from_numpy(mine).to(dev)
        g = od.allgather_shards(buf, world).cpu().numpy()  # [world, rows, D]
        return np.concatenate([g[r, : od.shard_bounds(total, r, world)[1] - od.shard_bounds(total, r, world)[0]] for r in range(world)])

    def _get(self, f):
        if f not in self._cache:
            self._cache[f] = self.ctx.get(f)
        return self._cache[f]

    # Adaptive solves keep one device record per ATTEMPTED step; a rejected attempt repeats the previous record at
    # the unchanged time (include/odefilter.h, odef_solve_adaptive).  The reference saves accepted steps only
    # (src/integrator_utils.jl:33-48), so the accessors below drop the repeats.
    def _order(self):
        """(order [N, n_save], count [N]): per trajectory the record indices with the kept ones first."""
        if "_order" not in self._cache:
            tt = self._tsave()
            ns = self._get(F_NSAVED)
            idx = np.arange(tt.shape[1])[None, :]
            keep = idx < ns[:, None]
            keep[:, 1:] &= tt[:, 1:] != tt[:, :-1]
            self._cache["_order"] = (np.argsort(~keep, axis=1, kind="stable"), keep.sum(axis=1).astype(np.int32))
        return self._cache["_order"]

    def _tsave(self) -> np.ndarray:
        """Adaptive solves: the per-trajectory save times [N, n_save] (also for N = 1)."""
        return self._get(F_T).reshape(self.ctx.n_save, self.ctx.N).T

    def raw_index(self, i: int) -> np.ndarray:
        """Device record index of every kept record of trajectory i (identity for fixed grids)."""
        if not self.adaptive:
            return np.arange(self.ctx.n_save)
        order, count = self._order()
        return order[i, : count[i]]

    def _compact(self, a: np.ndarray) -> np.ndarray:
        """a: [N, n_save, ...] -> same shape, kept records first, the rest zero."""
        if not self.adaptive:
            return a
        order, count = self._order()
        out = np.take_along_axis(a, order.reshape(order.shape + (1,) * (a.ndim - 2)), axis=1)
        out[np.arange(a.shape[1])[None, :] >= count[:, None]] = 0
        return out

    @property
    def t(self) -> np.ndarray:
        """Fixed grid: [n_save] (shared by all trajectories); adaptive: [N, n_save], zero-padded."""
        return self._compact(self._tsave()) if self.adaptive else self._get(F_T).reshape(-1)

    @property
    def nsaved(self) -> np.ndarray:
        return self._order()[1] if self.adaptive else self._get(F_NSAVED)

    def x_filt_mean(self) -> np.ndarray:
        return self._compact(self._get(F_MEAN).transpose(2, 0, 1))

    def x_filt_cov(self) -> np.ndarray:
        return unpack_tril(self._compact(self._get(F_COV_TRIL).transpose(2, 0, 1)), self.D)

    def x_smooth_mean(self) -> np.ndarray:
        return self._compact(self._get(F_SMOOTH_MEAN).transpose(2, 0, 1))

    def x_smooth_cov(self) -> np.ndarray:
        return unpack_tril(self._compact(self._get(F_SMOOTH_COV_TRIL).transpose(2, 0, 1)), self.D)

    @property
    def smoothed(self) -> bool:
        return bool(self.alg.smooth) and self.ctx.cfg.save_mode == SAVE_EVERYSTEP

    @property
    def u(self) -> np.ndarray:
        """sol.u: posterior mean of the solution, smoothed when alg.smooth (src/integrator_utils.jl:20-26)."""
        m = self.x_smooth_mean() if self.smoothed else self.x_filt_mean()
        return m[:, :, : self.d]

    @property
    def pu_cov(self) -> np.ndarray:
        """Covariance of sol.pu = SolProj * x (src/integrator_utils.jl:21,45)."""
        c = self.x_smooth_cov() if self.smoothed else self.x_filt_cov()
        return c[:, :, : self.d, : self.d]

    def __call__(self, t, smoothed: Optional[bool] = None):
        """`sol(t)`: dense output (src/solution.jl:211-215).  Returns (mean [N, n_t, D], cov [N, n_t, D, D]) of the
        posterior at the times `t` (smoothed when the solution is, as the reference's interpolant)."""
        tq = np.atleast_1d(np.asarray(t, float))
        sm = self.smoothed if smoothed is None else smoothed
        m, c = self.ctx.dense_output(tq, sm)
        return m.transpose(2, 0, 1), unpack_tril(c.transpose(2, 0, 1), self.D)

    @property
    def errors(self):
        """sol.errors (src/solution.jl:11, 68-74): dict with "l∞", "l2", "final" -- DiffEqBase's timeseries errors of sol.u (the
        smoothed means when the solution is smoothed) against the truth -- plus "chi2", each [N], computed on the device.  None
        when the vector field has no `analytic` and no reference is bound, as the reference returns `nothing`."""
        if "errors" not in self._cache:
            try:
                e = self.ctx.solution_errors(E_SOURCE_SMOOTH if self.smoothed else E_SOURCE_FILTER)
                e.pop("nused")
            except OdefError as ex:
                if _NO_TRUTH not in str(ex):
                    raise
                e = None
            self._cache["errors"] = e
        return self._cache["errors"]

    @property
    def u_analytic(self):
        """sol.u_analytic (src/solution.jl:10): the truth at every trajectory's own save times, [N, n_save, d] like `u`; None
        without a truth."""
        if "u_analytic" not in self._cache:
            try:
                a = self.ctx.get(errors_field(E_SOURCE_SMOOTH if self.smoothed else E_SOURCE_FILTER, E_U_ANALYTIC))
                a = self._compact(a.transpose(2, 0, 1))
            except OdefError as ex:
                if _NO_TRUTH not in str(ex):
                    raise
                a = None
            self._cache["u_analytic"] = a
        return self._cache["u_analytic"]

    def data_loglik(self, times, data, noise_var, components=None):
        """Log-likelihood of noisy observations of the solution per trajectory, on the device: for y_j = u(times[j])[components] +
        N(0, diag noise_var), the marginal likelihood under the Gauss-Markov posterior the filter records and the smoother's
        backward transitions define (Tronarp, Bosch, Hennig 2022; later versions of the reference: `fenrir_data_loglik`).
        `times` are strictly increasing, from t0 on; `data` is [M, o] (shared) or [N, M, o]; `noise_var` a scalar or [o];
        `components` defaults to all d.  Returns (loglik [N], mahalanobis [N]): with per-trajectory u0 or p, argmax of the first
        is the candidate that explains the data best; the second is chi^2 with M o degrees of freedom for a calibrated model.
        After a fixed-grid solve whose `times` all equal entries of `sol.t` the sweep runs over the saves; otherwise -- times off
        the grid (up to its last save), or an adaptive solve -- over every trajectory's own records with the filter's prediction
        inserted at each time that is no save.  A trajectory of an adaptive solve whose records end before the last time gets NaN."""
        by_time = self.adaptive or not _on_grid(self.t, times)
        if by_time:
            t = None if self.adaptive else self.t
            arrays = _observation_time_arrays(self.d, self.ctx.N, times, data, noise_var, components,
                                              None if t is None else t[0], None if t is None else t[-1])
        else:
            arrays = _observation_arrays(self.t, self.d, self.ctx.N, times, data, noise_var, components)
        self._obs_bufs = _to_device(arrays[:4], self.ctx.cfg.device)  # device memory owned by torch, kept alive by the solution
        return Context._data_loglik(self.ctx.lib, self.ctx._h, self._obs_bufs, by_time)

    def events(self, component, level=0.0, direction=0, max_events=1, smoothed: Optional[bool] = None) -> Events:
        """When does each trajectory cross a level?  The times at which component `component` of the posterior mean crosses
        `level` (a scalar, or [N] per trajectory) -- the answer of a `ContinuousCallback` with condition u[c] - level, asked of the
        finished posterior, on the device.  direction +1 keeps upward crossings, -1 downward, 0 both; the first `max_events` per
        trajectory are located, `count` counts all.  Works on fixed and adaptive grids (`save` is then a raw record index,
        `raw_index`).  smoothed=None: the smoothed posterior if the solution is smoothed.  The state carries u', so the root is
        found by Newton on the dense posterior mean without extra evaluations of the field, and the posterior variance at the
        root gives `t_std`.  A crossing that does not show at the two ends of a step (a double root inside one step) is not
        detected.  On the filter posterior (smoothed=False) the interpolant jumps at every save by the measurement update; a
        crossing that happens inside such a jump is reported at the save itself, with the stored state.  Returns `Events`."""
        sm = self.smoothed if smoothed is None else bool(smoothed)
        arrays = _event_arrays(self.d, self.ctx.N, component, level, direction, max_events)
        self._event_bufs = _to_device(arrays, self.ctx.cfg.device)  # device memory owned by torch, kept alive by the solution
        return Context._events(self.ctx.lib, self.ctx._h, self.ctx, int(sm), self._event_bufs)

    def _no_sharded_quantiles(self):
        if self.shard is not None and self.shard[3] > 1:
            raise OdefError("quantiles of a sharded ensemble: the quantiles of the shards do not pool into those of the whole "
                            "ensemble (exact pooling would all-reduce the per-pass histograms, which is not built); "
                            "solve the ensemble on one device, or gather the means")

    def _quantile_source(self, t, smoothed, who="quantiles()", taken="the quantiles of the dense output are taken"):
        """Evaluates the dense output when t is given; returns (times, source) by the rules of `summary()`."""
        sm = self.smoothed if smoothed is None else bool(smoothed)
        if t is None:
            if self.adaptive:
                raise OdefError(f"{who}: an adaptive solve keeps its records at different times per trajectory; "
                                f"pass common times t ({taken})")
            return self.t, (S_SOURCE_SMOOTH if sm else S_SOURCE_FILTER)
        tt = np.ascontiguousarray(np.atleast_1d(np.asarray(t, float)))
        self.ctx._chk(self.ctx.lib.odef_dense_output(self.ctx._h, _as_dp(tt), len(tt), int(sm)))
        return tt, S_SOURCE_DENSE

    def quantiles(self, probs, t=None, smoothed: Optional[bool] = None) -> np.ndarray:
        """[n_t, P, d]: the quantiles `probs` (1 to 8 values in [0, 1]) of every solution component of the posterior means over
        the ensemble, per time, selected on the device (`odef_quantile_field`) -- the median and the credible bands that
        `mean +- std` cannot give for a skewed or bimodal ensemble.  Type-7 rule (numpy's default), exact.  t, smoothed and
        adaptive solves: the rules of `summary()`.  Trajectories are included as in `summary()`; a time without any gives NaN.
        The quantiles of a sharded ensemble are refused."""
        self._no_sharded_quantiles()
        _, source = self._quantile_source(t, smoothed)
        return self.ctx.ensemble_quantiles(source, probs)[1]

    def summary(self, t=None, smoothed: Optional[bool] = None, quantiles=None, log_weights=None) -> EnsembleSummary:
        """Mean path of the ensemble and its uncertainty, reduced on the device (`odef_summary_field`): nothing but the four
        small arrays crosses to the host.  t = None: the save grid of a fixed-grid solve, smoothed when the solution is (the rule
        of `sol.u`).  With t: the dense output `sol(t)` is evaluated on the device and summarised.  Adaptive solves need t (their
        records of one save index lie at different times per trajectory).  A distributed solve returns the summary of the WHOLE
        ensemble on every rank: one all_gather of the per-shard blocks, pooled with `merge_moments`.  quantiles=(lo, hi): the
        summary also carries `qlow`, `med`, `qhigh` [n_t, d] (`quantiles()` with (lo, 0.5, hi), one pass); not for sharded solves.
        log_weights [N] (this rank's trajectories; a distributed solve also takes the whole ensemble's and cuts its block): the
        mixture is weighted by w_i proportional to exp(log_weights_i) (`odef_wsummary_field`; a value that is not finite excludes
        its trajectory) and the summary carries `ess` and `log_evidence`; the shards of a distributed solve pool with
        `merge_weighted_moments`.  Not together with quantiles."""
        if log_weights is not None:
            return self._weighted_summary(t, smoothed, quantiles, log_weights)
        if quantiles is not None:
            self._no_sharded_quantiles()
        sm = self.smoothed if smoothed is None else bool(smoothed)
        if t is None:
            if self.adaptive:
                raise OdefError("summary(): an adaptive solve keeps its records at different times per trajectory; "
                                "pass common times t (the dense output is summarised)")
            tt = self.t
            moments = self.ctx.ensemble_moments(S_SOURCE_SMOOTH if sm else S_SOURCE_FILTER)
        else:
            tt = np.ascontiguousarray(np.atleast_1d(np.asarray(t, float)))
            self.ctx._chk(self.ctx.lib.odef_dense_output(self.ctx._h, _as_dp(tt), len(tt), int(sm)))
            moments = self.ctx.ensemble_moments(S_SOURCE_DENSE)
        if self.shard is not None and self.shard[3] > 1:
            from . import dist as od

            moments = merge_moments(od.allgather_moments(moments, self.shard[3]))
        out = EnsembleSummary.from_moments(tt, *moments)
        if quantiles is not None:  # the dense records of `t` are still those just summarised
            lo, hi = (float(v) for v in quantiles)
            q = self.ctx.ensemble_quantiles(S_SOURCE_DENSE if t is not None else S_SOURCE_SMOOTH if sm else S_SOURCE_FILTER,
                                            (lo, 0.5, hi))[1]
            out.qlow, out.med, out.qhigh, out.quantile_probs = q[:, 0], q[:, 1], q[:, 2], (lo, hi)
        return out

    _BOUND_WEIGHTS = object()  # `_weighted_summary`: the log-weights the context holds already

    def _weighted_summary(self, t, smoothed, quantiles, log_weights) -> EnsembleSummary:
        if quantiles is not None:
            raise OdefError("summary(quantiles=..., log_weights=...): weighted quantiles are not built (they would need integer "
                            "fixed-point weights in the radix histograms to stay exact); ask for one of the two")
        sharded = self.shard is not None and self.shard[3] > 1
        if log_weights is not self._BOUND_WEIGHTS:
            if hasattr(log_weights, "detach"):  # a torch tensor: cut to the rank's block like an array
                log_weights = log_weights.detach().cpu().numpy()
            log_weights = np.asarray(log_weights, float).reshape(-1)
            if sharded and log_weights.size == self.shard[2] != self.ctx.N:
                log_weights = log_weights[self.shard[0]:self.shard[1]]
        tt, source = self._quantile_source(t, smoothed, "summary()", "the dense output is summarised")  # (the rules of `summary()`, and its dense output)
        moments = self.ctx.weighted_moments(source, None if log_weights is self._BOUND_WEIGHTS else log_weights)
        if sharded:
            from . import dist as od

            moments = merge_weighted_moments(od.allgather_weighted_moments(moments, self.shard[3]))
        return EnsembleSummary.from_moments(tt, *moments)

    def posterior_predictive(self, times, data, noise_var, components=None, log_prior=None, t=None,
                             smoothed: Optional[bool] = None) -> EnsembleSummary:
        """What the ensemble predicts given noisy measurements: `data_loglik(times, data, noise_var, components)` per
        trajectory, plus `log_prior` [N] if given, as the log-weights of `summary(t, smoothed, log_weights=...)`.  The weights
        stay on the device (a device-to-device copy of the likelihood into a tensor the context owns).  With candidates drawn
        from the prior, `log_evidence` is the Monte-Carlo log marginal likelihood of the data and `ess` says how many candidates
        still carry weight.  A trajectory the likelihood could not score (NaN) is left out."""
        self.data_loglik(times, data, noise_var, components)
        if log_prior is not None and self.shard is not None and self.shard[3] > 1:
            log_prior = np.asarray(log_prior, float).reshape(-1)
            if log_prior.size == self.shard[2] != self.ctx.N:
                log_prior = log_prior[self.shard[0]:self.shard[1]]
        self.ctx.bind_data_loglik_as_weights(log_prior)
        return self._weighted_summary(t, smoothed, None, self._BOUND_WEIGHTS)

    def sample_states(self, n: int = 1, seed: int = 0x5A3B1E, noise_scale: float = 1.0) -> np.ndarray:
        """`sample_states(sol, n)` (src/solution_sampling.jl:15-18, 24-62): [N, n_save, D, n] joint draws of the
        state path from the smoothing posterior.  The reference asserts a smoothing solve (:16)."""
        if not self.smoothed:
            raise AssertionError("sampling not implemented for non-smoothed posteriors")
        return self._compact(self.ctx.sample_states(n, seed, noise_scale).transpose(3, 0, 1, 2))

    def sample(self, n: int = 1, seed: int = 0x5A3B1E) -> np.ndarray:
        """`sample(sol, n)` (src/solution_sampling.jl:19-23): [N, n_save, d, n]."""
        return self.sample_states(n, seed)[:, :, : self.d, :]

    def dense_sample_states(self, n: int = 1, seed: int = 0x5A3B1E, times=None, noise_scale: float = 1.0):
        """`dense_sample_states(sol, n)` (src/solution_sampling.jl:63-69): ([N, n_t, D, n], times); the reference's
        grid is range(t0, t_end, length=1000), any non-decreasing `times` in [t0, t_end] may be given instead."""
        if not self.smoothed:
            raise AssertionError("sampling not implemented for non-smoothed posteriors")
        if times is None:
            t = self.t
            t0, t_end = (t[0, 0], t[0, self.nsaved[0] - 1]) if self.adaptive else (t[0], t[-1])
            times = np.linspace(float(t0), float(t_end), 1000)
        times = np.ascontiguousarray(times, float)
        return self.ctx.dense_sample_states(times, n, seed, noise_scale).transpose(3, 0, 1, 2), times

    def dense_sample(self, n: int = 1, seed: int = 0x5A3B1E, times=None):
        """`dense_sample(sol, n)` (src/solution_sampling.jl:70-75): ([N, n_t, d, n], times)."""
        s, times = self.dense_sample_states(n, seed, times)
        return s[:, :, : self.d, :], times

    @property
    def diffusions(self) -> np.ndarray:
        """[N, n_save-1]: entry k = diffusion of step t[k] -> t[k+1] (src/integrator_utils.jl:44); the MV models:
        [N, n_save-1, d], the diagonal of that diffusion."""
        if self.ctx.mv:
            return self._compact(self._get(F_DIFFUSION).transpose(2, 0, 1))[:, 1:]
        return self._compact(self._get(F_DIFFUSION).T)[:, 1:]

    @property
    def log_likelihood(self) -> np.ndarray:
        return self._get(F_LOGLIK)

    @property
    def destats(self) -> DEStats:
        return DEStats(self._get(F_NF), self._get(F_NJAC), self._get(F_NACCEPT), self._get(F_NREJECT))

    @property
    def retcode(self):
        return [RETCODES[int(r)] for r in self._get(F_RETCODE)]

    @property
    def retcode_raw(self) -> np.ndarray:
        return self._get(F_RETCODE)


def solve(prob, alg, ensemblealg: EnsembleHIP = EnsembleHIP(), *, trajectories: Optional[int] = None,
          dt: Optional[float] = None, adaptive: bool = True, abstol: float = 1e-6, reltol: float = 1e-3,
          tstops: Optional[Sequence[float]] = None, save_everystep: bool = True, maxiters: int = 100000,
          max_steps: Optional[int] = None, want_loglik: bool = True) -> EnsembleSolution:
    """`solve(EnsembleProblem(prob), EK1(order=3), EnsembleHIP(); trajectories, dt, adaptive, abstol, reltol)`.

    Keyword meaning follows DifferentialEquations.jl: `adaptive=false` needs `dt` (steps clipped onto `tstops` and the
    end of the time span) or `tstops` alone as the full grid; with `adaptive=true`, `dt` is the initial step.

    Differences from the reference's defaults, stated: (i) without `dt` an adaptive solve starts with 1e-3 (t1 - t0),
    not with OrdinaryDiffEq's automatic initial step (that heuristic evaluates `f` on the host; the vector field
    lives on the device) -- `sol.t` / `destats` then differ from the reference's, the posterior at common times does
    not beyond the tolerances; (ii) the device keeps one record per ATTEMPTED step, so the step budget is
    `max_steps` (default: `maxiters`, capped so that the records stay below 8 GiB); a trajectory that exhausts it ends
    with retcode MaxIters and a RuntimeWarning is raised, as for any other non-Success retcode."""
    if isinstance(prob, ODEProblem):
        prob = EnsembleProblem(prob, u0s=np.asarray(prob.u0, float)[None, :])
        trajectories = 1
    shard = None
    if ensemblealg.distributed:
        from . import dist as od

        rank, world, local_rank = od.init_from_env(backend=ensemblealg.backend)
        if ensemblealg.backend == "nccl":
            import torch

            torch.cuda.set_device(local_rank if ensemblealg.device < 0 else ensemblealg.device)
        total = len(prob.u0s) if prob.u0s is not None else trajectories
        prob, trajectories, (lo, hi) = shard_ensemble(prob, trajectories, rank, world)
        if hi == lo:
            raise OdefError(f"rank {rank} of {world} received no trajectory (ensemble of {total})")
        shard = (lo, hi, int(total), world)
        if ensemblealg.device < 0:
            ensemblealg = EnsembleHIP(device=local_rank, distributed=True, backend=ensemblealg.backend)
    base = prob.prob
    if alg.prior != "ibm":
        raise OdefError("Only the ibm prior is implemented so far")  # src/caches.jl:69
    if alg.diffusionmodel not in DIFFUSION:
        raise OdefError(f"diffusionmodel {alg.diffusionmodel!r} is not on the device path; use one of {sorted(DIFFUSION)}")
    if alg.diffusionmodel in MV_DIFFUSIONS and alg._id != EK0_ID:
        raise OdefError("MV diffusion models require EK0")  # src/diffusions.jl:96, :125
    lin_sol = getattr(alg, "linearize_at", None)
    if lin_sol is not None and adaptive:
        raise OdefError("IEKS relinearisation runs on fixed grids: pass adaptive=False and dt (or tstops)")
    if not adaptive and dt is None and tstops is None:
        # test/errors.jl:17-19
        raise OdefError("Fixed timestep methods require a choice of dt or choosing the tstops")
    if prob.u0s is not None:
        u0s = np.ascontiguousarray(prob.u0s, float)
        N = u0s.shape[0]
        if trajectories is not None and trajectories != N:
            raise OdefError(f"trajectories={trajectories} but u0s has {N} rows")
    else:
        if trajectories is None:
            raise OdefError("trajectories is required")
        N = trajectories
    t0, t1 = float(base.tspan[0]), float(base.tspan[1])
    if lin_sol is not None and lin_sol.ctx.N != N:
        raise OdefError(f"IEKS: linearize_at holds {lin_sol.ctx.N} trajectories, this ensemble has {N}")
    shared = prob.ps is None
    ctx = Context(base.f, alg.order, alg._id, N, diffusion=alg.diffusionmodel, smooth=alg.smooth,
                  save_everystep=save_everystep, params_shared=shared, device=ensemblealg.device,
                  want_loglik=want_loglik)
    p = np.asarray(base.p, float).reshape(-1) if shared else np.asarray(prob.ps, float)
    if prob.u0s is not None:
        ctx.set_problem(u0s, p, t0)
    else:
        if prob.perturb_scale is None:
            raise OdefError("EnsembleProblem needs u0s or perturb_scale")
        ctx.set_problem_perturbed(base.u0, p, t0, prob.perturb_scale, prob.seed, prob.first_index, prob.n_perturbed)
    if not (t1 > t0):
        raise OdefError(f"tspan must be increasing, got ({t0!r}, {t1!r})")
    if adaptive:
        if dt is not None and not (np.isfinite(dt) and dt > 0.0):
            raise OdefError(f"dt must be positive and finite, got {dt!r}")
        if max_steps is not None:
            ms = int(max_steps)
        else:  # maxiters attempts, bounded by the memory of one record per attempt
            rec_bytes = 8 * (ctx.D + ctx.TRI + 2) * (2 if alg.smooth else 1)
            ms = int(max(64, min(int(maxiters), (8 << 30) // (rec_bytes * N))))
        ctx.solve_adaptive(t1, abstol, reltol, dt if dt is not None else 1e-3 * (t1 - t0), None, ms)
    else:
        grid = np.asarray(tstops, float) if (tstops is not None and dt is None) else fixed_time_grid(t0, t1, dt, tstops)
        if lin_sol is not None:
            _bind_linearization(ctx, lin_sol, grid)
        ctx.solve_fixed(grid)
    sol = EnsembleSolution(ctx, alg, adaptive)
    sol.shard = shard
    if alg.smooth and ctx.cfg.save_mode == SAVE_EVERYSTEP:
        ctx.smooth()
    bad = np.flatnonzero(sol.retcode_raw != 0)
    if bad.size:
        import warnings

        kinds = sorted({RETCODES[int(r)] for r in sol.retcode_raw[bad]})
        warnings.warn(f"{bad.size} of {N} trajectories did not finish with Success ({', '.join(kinds)}; first: trajectory "
                      f"{int(bad[0])}); see sol.retcode", RuntimeWarning, stacklevel=2)
    return sol


def _bind_linearization(ctx: Context, lin_sol: EnsembleSolution, grid: np.ndarray) -> None:
    """IEKS(linearize_at = lin_sol): bind the smoothed u of `lin_sol` on `grid` as ODEF_F_LINEARIZE_AT [n_t][d][N] -- its
    smoothed records when it was solved on this grid (linearize_at(t) at a save time is that record), else its smoothed dense
    output `lin_sol(grid)`.  The buffer is device memory owned by torch, kept alive by the context."""
    import torch

    same = not lin_sol.adaptive and lin_sol.t.shape == grid.shape and np.array_equal(lin_sol.t, grid)
    u = lin_sol.x_smooth_mean() if same else lin_sol(grid, smoothed=True)[0]  # [N, n_t, D]
    lin = np.ascontiguousarray(u[:, :, : ctx.d].transpose(1, 2, 0))
    dev = int(ctx.cfg.device) if ctx.cfg.device >= 0 else torch.cuda.current_device()
    buf = torch.from_numpy(lin).to(torch.device("cuda", dev))
    torch.cuda.synchronize(dev)
    ctx.bind_device(F_LINEARIZE_AT, buf.data_ptr(), buf.numel() * 8)
    ctx._lin_buf = buf


def solve_ieks(prob, alg: IEKS, ensemblealg: EnsembleHIP = EnsembleHIP(), *, iterations: int = 10, **kw) -> EnsembleSolution:
    """`solve_ieks(prob, IEKS(...); iterations=10, kwargs...)` (src/ieks.jl:52-61): `iterations` complete solves (filter,
    postamble, smoother) of the same problem on one fixed grid, each linearising at the previous one's smoothed u, with no
    stopping criterion.  The first iteration is EK1 whatever `alg.linearize_at` holds, as in the reference's loop.  Every
    iteration reuses one device context: the smoother leaves the next linearisation points on the device
    (ODEF_F_LINEARIZE_AT), nothing goes through the host between iterations.  The result is the last iteration's solution
    (its destats and log-likelihood are that solve's), with `sol.alg` = `alg`.  Fixed grids only (`adaptive=False` with `dt`
    or `tstops`): relinearising an adaptive solve is out of scope."""
    if not isinstance(alg, IEKS):
        raise OdefError("solve_ieks needs an IEKS algorithm")
    if kw.get("adaptive", True):
        raise OdefError("IEKS relinearisation runs on fixed grids: solve_ieks needs adaptive=False and dt (or tstops)")
    if int(iterations) < 1:
        raise OdefError("solve_ieks: iterations must be >= 1")
    first = IEKS(prior=alg.prior, order=alg.order, diffusionmodel=alg.diffusionmodel)  # sol = nothing (src/ieks.jl:56)
    sol = solve(prob, first, ensemblealg, **kw)
    ctx, grid = sol.ctx, np.asarray(sol.t, float)
    for _ in range(int(iterations) - 1):  # alg.linearize_at = sol; sol = solve(prob, alg) -- on the device
        ctx.solve_fixed(grid)
        ctx.smooth()
    out = EnsembleSolution(ctx, alg, False)
    out.shard = sol.shard
    return out
