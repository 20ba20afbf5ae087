"""Reference of the ensemble quantiles (include/odefilter.h, odef_quantile_field): the definition in numpy.  Per time the
trajectories with retcode 0 and d finite solution entries of the mean are included; per (time, component) their values are sorted
and Q = x_(lo) if g == 0 else x_(lo) + g (x_(hi) - x_(lo)) with h = (n-1) p, lo = min(floor(h), n-1), hi = min(lo+1, n-1),
g = h - lo.  numpy rounds the difference, the product and the sum once each, as the device does, so results compare with ==
(np.testing.assert_array_equal: NaN positions equal, -0 equals +0).  Test infrastructure only."""
import numpy as np

PROBS8 = np.array([0.95, 0.0, 0.5, 1.0 / 3.0, 0.05, 1.0, 0.25, 0.75])  # the eight probabilities of the tests, unsorted


def included(mean, retcode, d):
    """[n_t, N] bool: mean [n_t, D, N], retcode [N]."""
    return (np.asarray(retcode) == 0)[None, :] & np.all(np.isfinite(mean[:, :d, :]), axis=1)


def reference(mean, retcode, d, probs):
    """mean [n_t, D, N], retcode [N], probs [P] -> (count [n_t] int64, q [n_t, P, d])."""
    mean = np.asarray(mean, np.float64)
    probs = np.asarray(probs, np.float64).reshape(-1)
    n_t, P = mean.shape[0], probs.size
    inc = included(mean, retcode, d)
    count = inc.sum(axis=1).astype(np.int64)
    q = np.full((n_t, P, d), np.nan)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(n_t):
            n = int(count[s])
            if n == 0:
                continue
            h = np.float64(n - 1) * probs                     # one rounding
            lo = np.minimum(np.floor(h), n - 1).astype(np.int64)
            hi = np.minimum(lo + 1, n - 1)
            g = h - lo.astype(np.float64)                     # exact
            for a in range(d):
                x = np.sort(mean[s, a, inc[s]])
                xl, xh = x[lo], x[hi]
                diff = xh - xl
                prod = g * diff
                q[s, :, a] = np.where(g == 0.0, xl, xl + prod)
    return count, q


def keys(x):
    """Order-preserving uint64 keys of doubles: ~bits for a negative value (sign bit set), bits | 1<<63 otherwise."""
    b = np.ascontiguousarray(x, np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))


def expected_passes(mean, retcode, d, slab):
    """Digit passes the selection runs, summed over its slabs of `slab` times: a slab needs ceil(bits / 8) passes, bits the bit
    length of the widest row's key range kmax - kmin over the included values (0 for a row of equal values or without any)."""
    mean = np.asarray(mean, np.float64)
    inc = included(mean, retcode, d)
    total = 0
    for s0 in range(0, mean.shape[0], slab):
        bits = 0
        for s in range(s0, min(s0 + slab, mean.shape[0])):
            if inc[s].any():
                for a in range(d):
                    k = keys(mean[s, a, inc[s]])
                    bits = max(bits, int(int(k.max()) - int(k.min())).bit_length())
        total += -(-bits // 8)
    return total


def check(got, want, label=""):
    """got / want: (count, q).  Exact."""
    assert got[0].dtype == np.int64, (label, got[0].dtype)
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"{label}: count")
    assert got[1].shape == want[1].shape, (label, got[1].shape, want[1].shape)
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"{label}: quantiles")
