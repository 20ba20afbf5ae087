"""The ensemble summary in extended precision: the yardstick of the summary tests ("exact").

Two passes in np.longdouble over records in the device layout -- mean [n_t, D, N], cov_tril [n_t, TRI, N], retcode [N] --: the
count of the included trajectories, the mean of their means, the mean of their covariances (within) and the covariance of their
means (between, divisor n), over the solution part (rows 0..d-1, the first d(d+1)/2 packed covariance rows).  A trajectory is
included at a time when its retcode is 0 and its d mean entries there are finite.  Shares no code with the library's host layer
(`merge_moments` in particular)."""
import numpy as np

U = 2.0 ** -53


def tri(d):
    return d * (d + 1) // 2


def reference(mean, cov_tril, retcode, d):
    """(count [n_t] int64, mean [n_t, d], within [n_t, tri], between [n_t, tri]) as longdouble, plus the two magnitudes the
    tolerances need: mean_i |mu_ik| [n_t, d] and mean_i |Sigma_i,kl| [n_t, tri] over the included trajectories."""
    mean = np.asarray(mean)
    cov_tril = np.asarray(cov_tril)
    n_t, _, N = mean.shape
    T = tri(d)
    rows = [(k, l) for k in range(d) for l in range(k + 1)]
    cnt = np.zeros(n_t, np.int64)
    m = np.full((n_t, d), np.nan, np.longdouble)
    w = np.full((n_t, T), np.nan, np.longdouble)
    b = np.full((n_t, T), np.nan, np.longdouble)
    am = np.full((n_t, d), np.nan)
    aw = np.full((n_t, T), np.nan)
    ok_rc = np.asarray(retcode) == 0
    for s in range(n_t):
        mu = mean[s, :d, :]
        inc = ok_rc & np.all(np.isfinite(mu), axis=0)
        n = int(inc.sum())
        cnt[s] = n
        if n == 0:
            continue
        x = mu[:, inc].astype(np.longdouble)
        c = cov_tril[s, :T, :][:, inc].astype(np.longdouble)
        m[s] = x.sum(axis=1) / n
        w[s] = c.sum(axis=1) / n
        xc = x - m[s][:, None]
        for p, (k, l) in enumerate(rows):
            b[s, p] = (xc[k] * xc[l]).sum() / n
        am[s] = np.abs(x).sum(axis=1) / n
        aw[s] = np.abs(c).sum(axis=1) / n
    return cnt, m, w, b, am, aw


def check(got, ref, d, n_for_bound=None, label=""):
    """Asserts the derived tolerances, per time and entry, with u = 2^-53 and n = COUNT:
    MEAN (n + 2) u mean_i|mu_ik|, COV_WITHIN (n + 2) u mean_i|Sigma_i,kl| (a float64 sum in any order plus the division),
    COV_BETWEEN n u sqrt(B_kk B_ll) with B the reference's, exactly 0 for n = 1; NaN where n = 0.  Returns the worst ratios
    (error / bound) of the three moments, for records."""
    cnt, m, w, b, am, aw = ref
    g_cnt, g_m, g_w, g_b = got
    assert np.array_equal(np.asarray(g_cnt, np.int64), cnt), (label, g_cnt, cnt)
    T = tri(d)
    rows = [(k, l) for k in range(d) for l in range(k + 1)]
    diag = [k * (k + 1) // 2 + k for k in range(d)]
    worst = [0.0, 0.0, 0.0]
    for s in range(len(cnt)):
        n = int(cnt[s]) if n_for_bound is None else int(n_for_bound[s])
        if cnt[s] == 0:
            assert np.all(np.isnan(g_m[s])) and np.all(np.isnan(g_w[s])) and np.all(np.isnan(g_b[s])), (label, s)
            continue
        em = np.abs(g_m[s].astype(np.longdouble) - m[s]).astype(float)
        bm = (n + 2) * U * am[s]
        assert np.all(em <= bm), (label, "MEAN", s, em, bm)
        ew = np.abs(g_w[s].astype(np.longdouble) - w[s]).astype(float)
        bw = (n + 2) * U * aw[s]
        assert np.all(ew <= bw), (label, "COV_WITHIN", s, ew, bw)
        eb = np.abs(g_b[s].astype(np.longdouble) - b[s]).astype(float)
        if cnt[s] == 1:
            assert np.all(g_b[s] == 0.0), (label, "COV_BETWEEN n = 1", s, g_b[s])
        bd = np.array([float(b[s, diag[k]]) for k in range(d)])
        bb = np.array([n * U * np.sqrt(bd[k] * bd[l]) for (k, l) in rows])
        assert np.all(eb <= bb), (label, "COV_BETWEEN", s, eb, bb)
        for j, (e, bound) in enumerate(((em, bm), (ew, bw), (eb, bb))):
            nz = bound > 0
            if nz.any():
                worst[j] = max(worst[j], float((e[nz] / bound[nz]).max()))
    assert T == g_w.shape[1] == g_b.shape[1]
    return worst


def shard_bounds(total, world):
    """odef_shard_range's rule: contiguous blocks, the first total % world one longer."""
    base, rem = divmod(total, world)
    out, lo = [], 0
    for r in range(world):
        c = base + (1 if r < rem else 0)
        out.append((lo, lo + c))
        lo += c
    return out
