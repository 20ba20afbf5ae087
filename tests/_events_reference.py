"""TEST INFRASTRUCTURE: the definition of the event location (include/odefilter.h, odef_event_field) in numpy on top
of `oracle.dense_output`, and the bounds of the tests that use it.

  locate     the bracket rule on the stored means, the root of each of the first K brackets by PLAIN BISECTION TO ADJACENT DOUBLES
             (independent of Newton), the outputs from `dense_output` at the root
  newton     the bracketed Newton iteration as the device runs it, restated; returns the root and its evaluation count
  check      a device (or emulated) result against `locate` / `newton` at the bounds below

Bounds.  The project's dense-output bar is rtol 1e-9, atol 1e-12 on means and 1e-6 max|C| on covariances; carried to the time axis:
  time        |t_dev - t_ref| <= eps_k / |slope_ref| + 4 ulp(t_ref),  eps_k = 1e-9 max(|m_c[k]|, |m_c[k+1]|, |level|) + 1e-12
  residual    |oracle dense mean_c(t_dev) - level| <= eps_k + |slope| 4 ulp(t_dev)
  U           against oracle.dense_output at the DEVICE's time, rtol 1e-9, atol 1e-12
  TIME_VAR    against Sigma_cc / slope^2 of the same evaluation: 1e-6 max|C| / slope^2 + 2 (1e-9 + 1e-12 / |slope|) TIME_VAR
  NEVAL       <= 64, and <= the restated Newton's count + 2 (rounding can cost a step)
  an exact hit (g_{k+1} == 0): time, U and TIME_VAR equal the stored record bit for bit, NEVAL = 0
  a crossing inside the measurement update (filter source only: the interpolant jumps at every save, and the prediction from save k
  has not passed the level by t_{k+1}): there is no root, so none of the root bounds applies; the event is the save t_{k+1}, time and
  U equal the stored record bit for bit, NEVAL = 1 (the left limit), and plain bisection on the interpolant must end at t_{k+1} too
Every event of every trajectory is checked: no event is skipped."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import odefilter_oracle as orc  # noqa: E402

MAX_EVAL = 64
STEP_TOL = 2.0 ** -40
KEYS = ("count", "time", "tvar", "u", "direction", "save", "neval")


# ---- records <-> oracle solutions ---------------------------------------------------------------------------------------------------

def unpack(tril, D):
    out = np.zeros((D, D))
    il = np.tril_indices(D)
    out[il] = tril
    return out + np.tril(out, -1).T


def solution_from_records(t, mean, cov_tril, diff, d, q, smean=None, scov_tril=None, need=None):
    """An oracle `Solution` of ONE trajectory from records in the ABI layout (t [n], mean [n, D], cov_tril [n, TRI], diff [n] with
    slot k + 1 the diffusion of the step k -> k + 1), so that `oracle.dense_output` interpolates exactly what a device holds.
    `need`: the record indices whose covariance is factored (the ends of the brackets; the others keep a zero factor and are never
    interpolated from); None: all."""
    D = d * (q + 1)
    sol = orc.Solution(d=d, q=q)
    sol.t = [float(x) for x in t]

    def states(ms, cs):
        return [orc.SRGaussian(np.array(m, float), orc.lower_factor(unpack(c, D)) if need is None or k in need else np.zeros((D, D)))
                for k, (m, c) in enumerate(zip(ms, cs))]

    sol.x_filt = states(mean, cov_tril)
    sol.diffusions = [float(x) for x in diff[1:]]
    if smean is not None:
        sol.x_smooth = states(smean, scov_tril)
    return sol


def records_of(sols, smoothed=False, repeat_at=(), capacity=None):
    """Device-layout records of oracle solutions (one per trajectory; their lengths may differ: adaptive solves): mean [n, D, N],
    cov_tril [n, TRI, N], diff [n, N], t [n, N], nsaved [N] and, with `smoothed`, smean / scov.  `repeat_at`: record indices after
    which the record is planted again at the unchanged time (h = 0: a repeated tstop, the repeat of a rejected attempt).  Rows past a
    trajectory's own count hold -7 (never read as data)."""
    d, q = sols[0].d, sols[0].q
    D = d * (q + 1)
    il = np.tril_indices(D)
    cols = []
    for s in sols:
        mu, cov, t = list(s.means(False)), [c[il] for c in s.covs(False)], list(s.t)
        df = [0.0] + list(s.diffusions)
        sm = list(s.means(True)) if smoothed else None
        sc = [c[il] for c in s.covs(True)] if smoothed else None
        for k in sorted(repeat_at, reverse=True):
            for a in (mu, cov, t, df) + ((sm, sc) if smoothed else ()):
                a.insert(k + 1, a[k])
        cols.append((np.array(t), np.array(mu), np.array(cov), np.array(df), None if sm is None else np.array(sm),
                     None if sc is None else np.array(sc)))
    n = max(len(c[0]) for c in cols) if capacity is None else capacity
    N = len(cols)

    def stack(j, shape):
        out = np.full((n,) + shape + (N,), -7.0)
        for i, c in enumerate(cols):
            out[: len(c[0]), ..., i] = c[j]
        return np.ascontiguousarray(out)

    rec = dict(t=stack(0, ()), mean=stack(1, (D,)), cov=stack(2, (len(il[0]),)), diff=stack(3, ()),
               nsaved=np.array([len(c[0]) for c in cols], np.int32), d=d, q=q)
    if smoothed:
        rec["smean"], rec["scov"] = stack(4, (D,)), stack(5, (len(il[0]),))
    return rec


def trajectory(rec, i, near=None):
    """The oracle `Solution` of trajectory i of device-layout records (`records_of`, or arrays fetched from a device).  `near` =
    (component, level, smoothed): only the records at the ends of that event's brackets get their covariance factored."""
    n = int(rec["nsaved"][i])
    t = rec["t"][:n, i] if rec["t"].ndim == 2 else rec["t"][:n]
    sm = "smean" in rec and rec["smean"] is not None
    need = None
    if near is not None:
        c, level, smoothed = near
        m = (rec["smean"] if smoothed else rec["mean"])[:n, c, i]
        need = {j for k, _ in brackets(t, m, level, 0) for j in (k, k + 1)}
    return solution_from_records(t, rec["mean"][:n, :, i], rec["cov"][:n, :, i], rec["diff"][:n, i], rec["d"], rec["q"],
                                 rec["smean"][:n, :, i] if sm else None, rec["scov"][:n, :, i] if sm else None, need=need)


# ---- the definition -----------------------------------------------------------------------------------------------------------------

def brackets(t, m, level, direction):
    """[(k, +1 / -1)] of the whole trajectory: t [n], m [n] the stored means of the component."""
    out = []
    for k in range(len(t) - 1):
        if not t[k + 1] > t[k]:
            continue
        ga, gb = m[k] - level, m[k + 1] - level
        up, down = ga < 0 and gb >= 0, ga > 0 and gb <= 0
        if (up and direction >= 0) or (down and direction <= 0):
            out.append((k, 1 if up else -1))
    return out


def _stored(sol, smoothed):
    return sol.x_smooth if smoothed else sol.x_filt


def dense(sol, consts, tval, smoothed):
    return orc.dense_output(sol, consts, float(tval), smoothed=bool(smoothed))


def left_limit(sol, consts, k):
    """The mean of the FILTER interpolant at t_{k+1} from the left: the prediction from save k over the whole step (the goal_pred of
    oracle.dense_output with h1 = t_{k+1} - t_k).  The stored record k + 1 differs from it by the measurement update: the filter's
    dense mean jumps at every save; the smoothed one is continuous."""
    A, Q_L, precond, d, q = consts
    P = precond(sol.t[k + 1] - sol.t[k])
    Qh = orc.apply_diffusion(Q_L, sol.diffusions[k])
    return orc.linmap(1.0 / P, orc.predict(orc.linmap(P, sol.x_filt[k]), A, Qh)).mu


def in_the_update(sol, consts, c, level, k, smoothed):
    """True when the bracket k -> k + 1 of the stored FILTER means holds no root of the interpolant: the prediction has not passed the
    level by t_{k+1}, the crossing happens inside the measurement update.  The event is then the save t_{k+1} with its stored record."""
    if smoothed:
        return False
    neg = sol.x_filt[k].mu[c] - level < 0
    g = left_limit(sol, consts, k)[c] - level
    return not (g > 0 if neg else g < 0)


def bisect_root(sol, consts, c, level, k, smoothed):
    """The root of E[u_c(t)] - level in (t_k, t_{k+1}) by plain bisection until the bracket's ends are adjacent doubles."""
    a, b = sol.t[k], sol.t[k + 1]
    neg = _stored(sol, smoothed)[k].mu[c] - level < 0
    while True:
        mid = a + 0.5 * (b - a)
        if not a < mid < b:
            return b
        g = dense(sol, consts, mid, smoothed).mu[c] - level
        if g == 0:
            return mid
        if (g < 0) == neg:
            a = mid
        else:
            b = mid


def newton(sol, consts, c, level, k, smoothed):
    """The device's iteration, restated (events_kernels.h, event_refine_lane): (t*, evaluations)."""
    d = sol.d
    tk, tk1 = sol.t[k], sol.t[k + 1]
    xs = _stored(sol, smoothed)
    ga, gb = xs[k].mu[c] - level, xs[k + 1].mu[c] - level
    if gb == 0:
        return tk1, 0
    a, b, neg, tol = tk, tk1, ga < 0, STEP_TOL * (tk1 - tk)
    neval = 0
    if not smoothed:  # the left limit at t_{k+1} first: a crossing inside the update has no root; else it is the secant's right end
        neval = 1
        if in_the_update(sol, consts, c, level, k, smoothed):
            return tk1, 1
        gb = left_limit(sol, consts, k)[c] - level
    x = a - ga * ((b - a) / (gb - ga))
    if not a <= x <= b:
        x = 0.5 * (a + b)
    while True:
        mu = dense(sol, consts, x, smoothed).mu
        neval += 1
        g, s = mu[c] - level, mu[d + c]
        if g == 0 or neval >= MAX_EVAL:
            return x, neval
        if (g < 0) == neg:
            a = x
        else:
            b = x
        with np.errstate(all="ignore"):
            xn = x - g / s if s != 0 else np.nan
        if not (s != 0 and np.isfinite(s)) or not a <= xn <= b:
            xn = 0.5 * (a + b)
        if abs(xn - x) <= tol:
            return xn, neval + 1  # the outputs are one more evaluation, at the accepted time
        x = xn


def outputs_at(sol, consts, c, tval, smoothed):
    """(U [d], Sigma_cc, slope, max|C|) of the dense posterior at tval."""
    g = dense(sol, consts, tval, smoothed)
    C = g.cov()
    return g.mu[: sol.d].copy(), float(C[c, c]), float(g.mu[sol.d + c]), float(np.abs(C).max())


def locate(sol, c, level, direction, K, smoothed):
    """The definition for one trajectory: dict(count, events=[dict(k, direction, t, exact, u, var, slope, tvar, eps)] of the first K)."""
    consts = orc.make_consts(sol.d, sol.q)
    m = np.array([x.mu[c] for x in _stored(sol, smoothed)])
    br = brackets(np.asarray(sol.t), m, level, direction)
    ev = []
    for k, dr in br[:K]:
        exact = m[k + 1] - level == 0
        jump = not exact and in_the_update(sol, consts, c, level, k, smoothed)
        exact = bool(exact or jump)
        t = sol.t[k + 1] if exact else bisect_root(sol, consts, c, level, k, smoothed)
        u, var, slope, _ = outputs_at(sol, consts, c, t, smoothed)
        with np.errstate(divide="ignore"):
            tvar = var / (slope * slope)
        ev.append(dict(k=k, direction=dr, t=t, exact=bool(exact), jump=bool(jump), u=u, var=var, slope=slope, tvar=tvar,
                       eps=1e-9 * max(abs(m[k]), abs(m[k + 1]), abs(level)) + 1e-12))
    return dict(count=len(br), events=ev, consts=consts)


def check_trajectory(sol, got, c, level, direction, K, smoothed, label="", ref=None, stats=None):
    """One trajectory of a device (or emulated) result -- got: dict of KEYS with count scalar, time / tvar / direction / save / neval
    [K], u [K, d] -- against the definition, at the bounds of the module docstring.  `stats`: dict of lists that collects the ratios."""
    ref = locate(sol, c, level, direction, K, smoothed) if ref is None else ref
    consts, d = ref["consts"], sol.d
    assert int(got["count"]) == ref["count"], (label, int(got["count"]), ref["count"])
    nloc = min(ref["count"], K)
    for s in range(K):
        tag = (label, "slot", s)
        if s >= nloc:  # unused slots
            assert np.isnan(got["time"][s]) and np.isnan(got["tvar"][s]) and np.all(np.isnan(got["u"][s])), tag
            assert got["direction"][s] == 0 and got["save"][s] == -1 and got["neval"][s] == 0, tag
            continue
        e = ref["events"][s]
        assert got["save"][s] == e["k"] and got["direction"][s] == e["direction"], (tag, got["save"][s], e["k"])
        td, k = float(got["time"][s]), e["k"]
        if e["exact"]:
            rec = _stored(sol, smoothed)[k + 1]
            assert td == sol.t[k + 1] and got["neval"][s] == (1 if e["jump"] else 0), tag
            assert np.array_equal(got["u"][s], rec.mu[:d]), tag
            if e["jump"]:  # truly no root inside: plain bisection on the interpolant ends at the save as well
                assert bisect_root(sol, consts, c, level, k, smoothed) == sol.t[k + 1], tag
                if stats is not None:
                    stats["jumps"] = stats.get("jumps", 0) + 1
            continue
        slope = abs(e["slope"])
        bound_t = e["eps"] / slope + 4 * np.spacing(abs(e["t"]))
        assert sol.t[k] <= td <= sol.t[k + 1], tag
        assert abs(td - e["t"]) <= bound_t, (tag, "time", td, e["t"], abs(td - e["t"]), bound_t)
        u, var, sl, cmax = outputs_at(sol, consts, c, td, smoothed)
        resid = abs(dense(sol, consts, td, smoothed).mu[c] - level)
        bound_r = e["eps"] + abs(sl) * 4 * np.spacing(abs(td))
        assert resid <= bound_r, (tag, "residual", resid, bound_r)
        assert np.allclose(got["u"][s], u, rtol=1e-9, atol=1e-12), (tag, "u", got["u"][s], u)
        tv = var / (sl * sl)
        bound_v = 1e-6 * cmax / (sl * sl) + 2 * (1e-9 + 1e-12 / abs(sl)) * tv
        assert abs(float(got["tvar"][s]) - tv) <= bound_v, (tag, "tvar", float(got["tvar"][s]), tv, bound_v)
        _, nref = newton(sol, consts, c, level, k, smoothed)
        assert 1 <= got["neval"][s] <= MAX_EVAL and got["neval"][s] <= nref + 2, (tag, "neval", got["neval"][s], nref)
        if stats is not None:
            stats.setdefault("time", []).append(abs(td - e["t"]) / bound_t)
            stats.setdefault("residual", []).append(resid / bound_r)
            stats.setdefault("tvar", []).append(abs(float(got["tvar"][s]) - tv) / bound_v)
            stats.setdefault("neval", []).append(int(got["neval"][s]))
            stats.setdefault("slope", []).append(slope)
    return ref


def check(rec, out, c, levels, direction, K, smoothed, label="", stats=None, same_as=None):
    """A whole result in the ABI layout (out: count [N], time / tvar / direction / save / neval [K, N], u [K, d, N]) against the
    definition on the records `rec`.  levels: scalar or [N].  `same_as`: per trajectory the index of an earlier trajectory with the
    same records AND level (a tiled ensemble), whose reference is reused and whose result must be equal bit for bit."""
    N = out["count"].size
    lv = np.broadcast_to(np.asarray(levels, float), (N,))
    refs = {}
    for i in range(N):
        got = dict(count=out["count"][i], time=out["time"][:, i], tvar=out["tvar"][:, i], u=out["u"][:, :, i],
                   direction=out["direction"][:, i], save=out["save"][:, i], neval=out["neval"][:, i])
        j = i if same_as is None else int(same_as[i])
        if j != i:
            for key in KEYS:
                a, b = (out[key][i], out[key][j]) if key == "count" else (out[key][..., i], out[key][..., j])
                assert np.array_equal(a, b, equal_nan=True), (label, "lane", i, "differs from its twin", j, key)
            continue
        refs[i] = check_trajectory(trajectory(rec, i, near=(c, float(lv[i]), smoothed)), got, c, float(lv[i]), direction, K, smoothed, label=f"{label} traj {i}",
                                   stats=stats)
    return refs


def summarize(stats):
    if not stats or not stats.get("time"):
        return "no located event off a save"
    ne = np.array(stats["neval"])
    return (f"{len(ne)} events with a root ({stats.get('jumps', 0)} more inside an update): time error / bound max {max(stats['time']):.3g}, residual / bound max {max(stats['residual']):.3g}, "
            f"TIME_VAR error / bound max {max(stats['tvar']):.3g}, |slope| {min(stats['slope']):.3g} .. {max(stats['slope']):.3g}, "
            f"NEVAL max {ne.max()} median {int(np.median(ne))}")
