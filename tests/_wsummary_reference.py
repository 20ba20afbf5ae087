"""The weighted ensemble summary in extended precision: the yardstick of the weighted-summary tests.

Records in the device layout -- mean [n_t, D, N], cov_tril [n_t, TRI, N], retcode [N] -- and unnormalised log-weights l [N].
L = max l_i over the trajectories with retcode 0 and l_i finite; v_i = np.exp(l_i - L) in float64 (the subtraction is the same
IEEE operation as on the device, and both exp are specified to 1 ulp, so the device's v_i differ by at most 2u relative); from
there on np.longdouble.  A trajectory is included at a time when its retcode is 0, its d mean entries there are finite and l_i is
finite.  Shares no code with the library's host layer (`merge_weighted_moments` in particular)."""
import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def tri(d):
    return d * (d + 1) // 2


def reference(mean, cov_tril, retcode, logw, d):
    """dict: count [n_t] int64; mean [n_t, d], within, between [n_t, tri], log_evidence, ess [n_t] as longdouble; and the
    magnitudes the bounds need: am = sum_i w_i |mu_ik| [n_t, d], aw = sum_i w_i |Sigma_i,kl|, ab = sum_i w_i |c_ik c_il| [n_t, tri]
    with c_i = mu_i - m."""
    mean = np.asarray(mean)
    cov_tril = np.asarray(cov_tril)
    logw = np.asarray(logw, np.float64)
    n_t, _, N = mean.shape
    T = tri(d)
    rows = [(k, l) for k in range(d) for l in range(k + 1)]
    ok = (np.asarray(retcode) == 0) & np.isfinite(logw)
    L = logw[ok].max() if ok.any() else np.nan
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.where(ok, np.exp(logw - L), 0.0)  # float64
    out = {
        "count": np.zeros(n_t, np.int64),
        "mean": np.full((n_t, d), np.nan, LD), "within": np.full((n_t, T), np.nan, LD), "between": np.full((n_t, T), np.nan, LD),
        "log_evidence": np.full(n_t, np.nan, LD), "ess": np.full(n_t, np.nan, LD),
        "am": np.full((n_t, d), np.nan), "aw": np.full((n_t, T), np.nan), "ab": np.full((n_t, T), np.nan),
    }
    for s in range(n_t):
        mu = mean[s, :d, :]
        inc = ok & np.all(np.isfinite(mu), axis=0)
        n = int(inc.sum())
        out["count"][s] = n
        if n == 0:
            continue
        vi = v[inc].astype(LD)
        Z = vi.sum()
        if Z == 0:  # the trajectory that carries L is not included here and every other weight underflowed
            out["log_evidence"][s] = -np.inf
            continue
        w = vi / Z
        x = mu[:, inc].astype(LD)
        c = cov_tril[s, :T, :][:, inc].astype(LD)
        m = (w * x).sum(axis=1)
        out["mean"][s] = m
        out["within"][s] = (w * c).sum(axis=1)
        xc = x - m[:, None]
        for p, (k, l) in enumerate(rows):
            out["between"][s, p] = (w * xc[k] * xc[l]).sum()
            out["ab"][s, p] = float((w * np.abs(xc[k] * xc[l])).sum())
        out["log_evidence"][s] = LD(L) + np.log(Z) - np.log(LD(n))
        out["ess"][s] = Z * Z / (vi * vi).sum()
        out["am"][s] = (w * np.abs(x)).sum(axis=1).astype(float)
        out["aw"][s] = (w * np.abs(c)).sum(axis=1).astype(float)
    return out


NAMES = ("MEAN", "COV_WITHIN", "COV_BETWEEN", "LOG_EVIDENCE", "ESS")


def check(got, ref, d, label="", values=None):
    """Asserts the bounds of DESIGN.md 3.19 per time and entry, u = 2^-53, n = COUNT:
      MEAN, COV_WITHIN   2 (n + 4) u sum_i w_i |x_i|
      COV_BETWEEN (k,l)  2 (n + 4) u sum_i w_i |c_ik c_il| + beta_k beta_l, beta the MEAN bound
      ESS                3 (n + 4) u relative
      LOG_EVIDENCE       (n + 8) u + 2 u |value|
    NaN where the reference is NaN, -inf where it is -inf.  got: (count, mean, within, between, log_evidence, ess).  `ref` gives
    the magnitudes (and n); `values`, if given, is another reference dict whose values are compared instead (the unweighted one of
    the all-equal pattern).  Returns the worst error / bound per quantity, in the order of NAMES."""
    val = ref if values is None else values
    g_cnt, g_m, g_w, g_b, g_le, g_ess = got
    assert np.array_equal(np.asarray(g_cnt, np.int64), ref["count"]), (label, g_cnt, ref["count"])
    rows = [(k, l) for k in range(d) for l in range(k + 1)]
    worst = [0.0] * 5

    def cmp(j, s, g, want, bound):
        g, want, bound = np.atleast_1d(g), np.atleast_1d(want), np.atleast_1d(bound)
        err = np.abs(g.astype(LD) - want).astype(float)
        print(f"{label} s={s} {NAMES[j]}: worst error / bound = {np.max(err / np.where(bound > 0, bound, 1.0)):.3g}")
        assert np.all(err <= bound), (label, NAMES[j], s, err, bound)
        nz = bound > 0
        if nz.any():
            worst[j] = max(worst[j], float((err[nz] / bound[nz]).max()))

    for s in range(len(ref["count"])):
        n = int(ref["count"][s])
        if np.isnan(ref["ess"][s]):  # n = 0 (log evidence NaN) or Z = 0 (log evidence -inf)
            assert np.all(np.isnan(g_m[s])) and np.all(np.isnan(g_w[s])) and np.all(np.isnan(g_b[s])) and np.isnan(g_ess[s]), (label, s)
            want = ref["log_evidence"][s]
            assert np.isnan(g_le[s]) if np.isnan(want) else g_le[s] == -np.inf, (label, s, g_le[s])
            continue
        k = 2 * (n + 4) * U
        beta = k * ref["am"][s]
        cmp(0, s, g_m[s], val["mean"][s], beta)
        cmp(1, s, g_w[s], val["within"][s], k * ref["aw"][s])
        cmp(2, s, g_b[s], val["between"][s], k * ref["ab"][s] + np.array([beta[a] * beta[b] for a, b in rows]))
        cmp(3, s, g_le[s], val["log_evidence"][s], (n + 8) * U + 2 * U * abs(float(val["log_evidence"][s])))
        cmp(4, s, g_ess[s], val["ess"][s], 3 * (n + 4) * U * float(val["ess"][s]))
        assert 1.0 <= g_ess[s] * (1 + 1e-12) and g_ess[s] <= n * (1 + 1e-12), (label, "ESS range", s, g_ess[s], n)
    return worst
