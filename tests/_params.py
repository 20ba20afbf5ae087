"""Ensembles with per-trajectory parameters, shared by tests/test_params_emul.py (CPU) and tests/test_gpu_params.py.

Every kernel family loads its parameters with `pl[k] = P.p_shared ? P.p[k] : P.p[k * N + i]`.  A slip in `i`, in the
[n_params][N] layout or in the host code that builds it gives every trajectory a finite, well-conditioned solution of the
wrong ODE, so a test of that branch compares trajectory i with the oracle run on `ps[i]` -- and is only worth something when the
oracle itself tells the neighbouring parameter rows apart by far more than the tolerance (`assert_separated`)."""
import numpy as np

import _parity as P
import odefilter_oracle as orc

SPREAD = 0.05
# smallest relative distance, in the solution block, between the oracle's answers for two neighbouring parameter rows:
# 10^4 x P.U_RTOL, so that "the right row" and "any other row" are told apart with four orders of magnitude to spare
MIN_SEPARATION = 1e-6


def ensemble(vf, N, seed, u0_scale=1e-2, spread=SPREAD):
    """(u0s [N, d], ps [N, n_params]): the oracle's synthetic initial values and p (1 + spread x standard normal)."""
    rng = np.random.default_rng(seed)
    ps = np.asarray(vf.p, float)[None, :] * (1.0 + spread * rng.standard_normal((N, len(vf.p))))
    return orc.ensemble_u0(vf.u0, N, u0_scale), ps


def separation(a, b, d):
    """Relative distance of two [n, >= d] mean histories in the solution block (max-norm over the run, as P.block_err)."""
    n = min(len(a), len(b))
    return float(P.block_err(np.asarray(a)[:n, :d], np.asarray(b)[:n, :d], d)[0])


def assert_separated(solve_one, u0s, ps, trajs, d, what="", base=None):
    """`solve_one(u0, p)` -> [n, >= d] oracle means.  For each checked trajectory i: the same u0s[i] with the NEXT parameter
    row (cyclically) must move the solution block by at least MIN_SEPARATION.  `base(i)`: the means for (u0s[i], ps[i]) where the
    caller has them already.  Returns the smallest distance met."""
    N = len(ps)
    worst = np.inf
    for i in trajs:
        own = solve_one(u0s[i], ps[i]) if base is None else base(i)
        dist = separation(solve_one(u0s[i], ps[(i + 1) % N]), own, d)
        assert dist >= MIN_SEPARATION, f"{what}: rows {i} and {(i + 1) % N} of ps give solutions only {dist:.1e} apart; widen the spread"
        worst = min(worst, dist)
    return worst


def separation_adaptive(a, b, d):
    """Two adaptive oracle solutions (their step sequences differ as soon as the parameters do): relative distance over the
    common leading records, of the solution block of the filter means together with the save times."""
    n = min(len(a.t), len(b.t))
    xa = np.column_stack([a.means(smoothed=False)[:n, :d], np.asarray(a.t)[:n]])
    xb = np.column_stack([b.means(smoothed=False)[:n, :d], np.asarray(b.t)[:n]])
    return float(np.abs(xa - xb).max() / np.abs(xb).max())
