"""High-precision evaluation of the reference ALGORITHM (not of any float64 implementation of it): what do the EK1
filter and the RTS smoother of src/perform_step.jl / src/filtering.jl / src/smoothing.jl give in (near-)exact arithmetic?

The tolerances of the parity tests rest on this.  Float64 implementations of the reference arithmetic agree in the
solution components u = E0 mu to 1e-14, but NOT in the higher-derivative blocks of the state and in the covariances:
those are ill-conditioned in the reference's own formulation (the float64 oracle itself is 1e-8 / 3e-4 away from the
exact result there).  So "the device agrees with the oracle to x" is the wrong question for those blocks; the right one is
"is the device as close to the exact result as the oracle is".  This script computes the exact results:

  exact_lorenz_mp.npz    Lorenz-63, EK1(order=3), dt = 2^-9, 1 024 steps (BASELINE configs 2/3, trajectory 0 of the
                         ensemble), filter AND smoother, mpmath with 50 significant digits
  exact_pleiades_ld.npz  Pleiades, EK1(order=5), dt = 2^-10, 24 steps (BASELINE config 4 at test size, trajectory 0),
                         filter, numpy longdouble (x87 extended, 64-bit mantissa = 2 048 x finer than float64: D = 168
                         is out of reach for mpmath in a build-container minute, and 11 extra bits are enough to rank
                         two float64 results)
  exact_pleiades_{ek1q2,ek0q3,ek1q5,ek1q5_dt6}_smooth_ld.npz
                         Pleiades, 12 steps, trajectories 0 and 4, filter AND RTS smoother (D = 84, 112, 168), longdouble: what
                         the D = 168 kernels' parity tests are measured against (round 3; until then their tolerance was
                         calibrated on the float64 oracle's own spread, and the order-5 covariances were not compared at all)

  exact_small_<field>_<ek0|ek1>q<order>[_fixed]_ld.npz  (python tests/golden/make_exact.py --small)
                         every other instantiation of the lane and row-team filters and of the three small-state smoothers
                         (D = 4 ... 18, orders 1 ... 5, EK0, the `fixed` diffusion model, d = 2, a non-dyadic step): 64 steps,
                         trajectories 0-3 of ensemble_u0(u0, 4, 1e-2), filter AND smoother, covariances of every record,
                         diffusions and log-likelihood, longdouble (SMALL_CASES below)
  exact_lorenz96_{ek1q2,ek1q3,ek0q3,ek1q5}_smooth_ld.npz  (--small as well)
                         Lorenz-96 (d = 16) on the matrix-core kernels, 12 steps of dt = 2^-7, trajectories 0 and 5, the layout
                         of the Pleiades fixtures

  exact_model_[ieks_]<field>_<ek0|ek1>q<order>[_<model>]_ld.npz  (python tests/golden/make_exact.py --models)
                         the families with arithmetic of their own, in the layout of the small fixtures (_exact_cases.MODEL_CASES):
                         the `fixedMAP` diffusion model, the diagonal models `dynamicMV` / `fixedMV` of EK0 (d diffusions per step,
                         [traj, step, d]), the third iteration of solve_ieks, and the time-dependent field `forced` from t0 = 0.25
                         (tests/_time_reference.py); the float64 side of the yardstick is orc.solve, tests/_mv_reference.py and
                         tests/_ieks_reference.py

and, next to them, the float64 oracle's distance from them per derivative block and for the covariance.  Any
mathematically equivalent formulation gives the same exact result, so the recursion is written in the plain covariance
form (Sigma^- = A Sigma A' + sigma^2 Q, K = Sigma^- H' S^-1, Sigma = (I - K H) Sigma^- (I - K H)'; G = Sigma A' (Sigma^-)^-1)
in preconditioned coordinates.  (The Joseph form of the update matters even at 50 digits: Sigma^- - K S K' amplifies
rounding errors by ~6x per step on this problem and is useless after 60 steps.)

A fixture is only as sharp as the oracle's diffusion estimates are: where the residuals are rounding noise in float64 (Pleiades
order 5 at dt = 2^-10: 0.4 relative and worse) "the oracle's distance" is a lottery ticket.  The --small entry asserts the
admission condition max |sigma^2_oracle - sigma^2_exact| / sigma^2_exact <= 1e-4 for every fixture trajectory before it writes,
and so does --models (for the MV models: every component).

Run (build container, ~3 min):  python tests/golden/make_exact.py            the Lorenz-63 / Pleiades fixtures
                  (~1 min):     python tests/golden/make_exact.py --small    the small-state and Lorenz-96 fixtures
                  (~10 s):      python tests/golden/make_exact.py --models   fixedMAP, the MV models, IEKS, f(u, p, t)
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
import odefilter_oracle as orc  # noqa: E402
from _parity import block_err, cov_err  # noqa: E402
import _exact_cases as X  # noqa: E402
import _ieks_reference as ier  # noqa: E402
import _mv_reference as mvr  # noqa: E402
from _exact_cases import LORENZ96_CASES, SMALL_CASES, SMALL_NSTEPS, SMALL_NTRAJ, lorenz96_name, small_name  # noqa: E402


# ---------------------------------------------------------------------------------------------- mpmath, Lorenz-63
def lorenz_mp(u0, p, q, dt, nsteps, digits=50):
    import mpmath as mp

    mp.mp.dps = digits
    d, NB = 3, q + 1
    D = d * NB
    M = mp.matrix
    h = mp.mpf(dt)
    sig, rho, beta = [mp.mpf(float(x)) for x in p]  # the float64 parameter values, exactly

    def f(u):
        return [sig * (u[1] - u[0]), u[0] * (rho - u[2]) - u[1], u[0] * u[1] - beta * u[2]]

    def jac(u):
        return M([[-sig, sig, 0], [rho - u[2], -1, -u[0]], [u[1], u[0], -beta]])

    # Taylor-mode initial state (src/state_initialization.jl:2-53): series coefficients by the Lie recursion
    c = [[mp.mpf(float(x))] + [mp.mpf(0)] * q for x in u0]  # c[a][k]
    for k in range(q):
        def conv(x, y, n):
            return sum(x[j] * y[n - j] for j in range(n + 1))
        fx = sig * (c[1][k] - c[0][k])
        fy = rho * c[0][k] - conv(c[0], c[2], k) - c[1][k]
        fz = conv(c[0], c[1], k) - beta * c[2][k]
        for a, v in enumerate((fx, fy, fz)):
            c[a][k + 1] = v / (k + 1)
    m = M(D, 1)
    for k in range(NB):
        for a in range(d):
            m[k * d + a] = c[a][k] * mp.factorial(k)
    # prior (src/priors.jl:7-59) and preconditioner (src/preconditioning.jl:1-17)
    A = mp.eye(D)
    for i in range(1, q + 1):
        for j in range(d * (q + 1 - i)):
            A[j, j + d * i] = mp.mpf(1) / mp.factorial(i)
    Q = M(D, D)
    for col in range(NB):
        for row in range(NB):
            v = mp.mpf(1) / ((2 * q + 1 - row - col) * mp.factorial(q - row) * mp.factorial(q - col))
            for i in range(d):
                Q[row * d + i, col * d + i] = v
    Pd = [h ** (mp.mpf(j) - q - mp.mpf(1) / 2) for j in range(NB) for _ in range(d)]
    E0 = M(d, D)
    E1 = M(d, D)
    for a in range(d):
        E0[a, a] = 1
        E1[a, d + a] = 1
    Pm = mp.diag(Pd)
    PIm = mp.diag([1 / x for x in Pd])
    S_ = M(D, D)  # Sigma_0 = 0
    means, covs, diffs = [m.copy()], [S_.copy()], []
    for _ in range(nsteps):
        mt, X = Pm * m, Pm * S_ * Pm
        mp_ = A * mt
        up = E0 * (PIm * mp_)
        z = E1 * (PIm * mp_) - M(f([up[0], up[1], up[2]]))
        H = (E1 - jac([up[0], up[1], up[2]]) * E0) * PIm
        W = H * Q * H.T
        s2 = (z.T * mp.lu_solve(W, z))[0] / d
        Xp = A * X * A.T + s2 * Q
        C = Xp * H.T
        Sm = H * C
        K = C * mp.inverse(Sm)  # K = C S^-1 (50 digits: the explicit inverse is harmless)
        mf = mp_ - K * z
        IKH = mp.eye(D) - K * H
        Xf = IKH * Xp * IKH.T  # Joseph form: the plain Sigma^- - K S K' amplifies rounding errors ~6x per step (50 digits last 60 steps)
        m, S_ = PIm * mf, PIm * Xf * PIm
        means.append(m.copy()); covs.append(S_.copy()); diffs.append(s2)
    # RTS pass (src/smoothing.jl:4-63)
    sm, sc = [None] * (nsteps + 1), [None] * (nsteps + 1)
    sm[nsteps], sc[nsteps] = means[nsteps], covs[nsteps]
    sm[0], sc[0] = means[0], covs[0]
    for i in range(nsteps - 1, 0, -1):
        mt, X = Pm * means[i], Pm * covs[i] * Pm
        mpred = A * mt
        B = A * X * A.T + diffs[i] * Q
        G = X * A.T * mp.inverse(B)
        ms = mt + G * (Pm * sm[i + 1] - mpred)
        Ss = X + G * (Pm * sc[i + 1] * Pm - B) * G.T
        sm[i], sc[i] = PIm * ms, PIm * Ss * PIm
    tof = lambda v: np.array([float(x) for x in v])  # noqa: E731
    tom = lambda a: np.array([[float(a[i, j]) for j in range(D)] for i in range(D)])  # noqa: E731
    return (np.array([tof(x) for x in means]), np.array([tom(x) for x in covs]), np.array([tof(x) for x in sm]),
            np.array([tom(x) for x in sc]), np.array([float(x) for x in diffs]))


# ------------------------------------------------------------------------------ longdouble, any vector field (filter)
def chol_ld(S):
    n = S.shape[0]
    L = np.zeros_like(S)
    for j in range(n):
        s = S[j, j] - L[j, :j] @ L[j, :j]
        L[j, j] = np.sqrt(s)
        L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_spd_ld(S, B):
    """S^-1 B for SPD S, longdouble."""
    L = chol_ld(S)
    n = S.shape[0]
    Y = np.zeros_like(B)
    for i in range(n):
        Y[i] = (B[i] - L[i, :i] @ Y[:i]) / L[i, i]
    X = np.zeros_like(B)
    for i in range(n - 1, -1, -1):
        X[i] = (Y[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


class JetLD:
    """Truncated Taylor arithmetic on longdouble coefficients (the oracle's Jet is float64 by construction): just what the
    oracle's vector fields need -- +, -, *, division by a scalar, real powers."""

    def __init__(self, c):
        self.c = np.asarray(c, dtype=np.longdouble)

    @staticmethod
    def lift(x, n):
        if isinstance(x, JetLD):
            return x
        c = np.zeros(n, dtype=np.longdouble)
        c[0] = x
        return JetLD(c)

    def __add__(self, o):
        return JetLD(self.c + JetLD.lift(o, len(self.c)).c)

    __radd__ = __add__

    def __sub__(self, o):
        return JetLD(self.c - JetLD.lift(o, len(self.c)).c)

    def __rsub__(self, o):
        return JetLD(JetLD.lift(o, len(self.c)).c - self.c)

    def __mul__(self, o):
        if not isinstance(o, JetLD):
            return JetLD(self.c * np.longdouble(o))
        n = len(self.c)
        return JetLD([np.dot(self.c[: k + 1], o.c[k::-1]) for k in range(n)])

    __rmul__ = __mul__

    def __neg__(self):
        return JetLD(-self.c)

    def __truediv__(self, o):  # by a scalar only (u^3 / 3.0 of the FitzHugh-Nagumo field)
        assert not isinstance(o, JetLD)
        return JetLD(self.c / np.longdouble(o))

    def __pow__(self, a):
        n = len(self.c)
        out = np.zeros(n, dtype=np.longdouble)
        out[0] = self.c[0] ** np.longdouble(a)
        for k in range(1, n):
            s = np.longdouble(0)
            for j in range(1, k + 1):
                s += (np.longdouble(a) * j - (k - j)) * self.c[j] * out[k - j]
            out[k] = s / (k * self.c[0])
        return JetLD(out)


def pleiades_jac_ld(u):
    ld = np.longdouble
    x, y = u[0:7], u[7:14]
    J = np.zeros((28, 28), dtype=ld)
    J[0:7, 14:21] = np.eye(7)
    J[7:14, 21:28] = np.eye(7)
    for i in range(7):
        for j in range(7):
            if j == i:
                continue
            mj = ld(j + 1)
            dx, dy = x[j] - x[i], y[j] - y[i]
            r2 = dx * dx + dy * dy
            r3, r5 = r2 ** ld(-1.5), r2 ** ld(-2.5)
            axx = mj * (r3 - 3 * dx * dx * r5)
            axy = mj * (-3 * dx * dy * r5)
            ayy = mj * (r3 - 3 * dy * dy * r5)
            J[14 + i, j] += axx; J[14 + i, i] -= axx; J[14 + i, 7 + j] += axy; J[14 + i, 7 + i] -= axy
            J[21 + i, j] += axy; J[21 + i, i] -= axy; J[21 + i, 7 + j] += ayy; J[21 + i, 7 + i] -= ayy
    return J


def lorenz96_jac_ld(u):
    """oracle _l96_jac, whose float64 work array would round the longdouble arguments."""
    n = len(u)
    J = np.zeros((n, n), dtype=np.longdouble)
    for i in range(n):
        ip, im2, im1 = (i + 1) % n, (i - 2) % n, (i - 1) % n
        J[i, ip] += u[im1]
        J[i, im2] -= u[im1]
        J[i, im1] += u[ip] - u[im2]
        J[i, i] -= 1
    return J


def jac_ld(vf, u, p, t=0.0):
    """The field's Jacobian on longdouble arguments (and, for f(u, p, t), at the longdouble time t).  The oracle's own `vf.jac` where it builds the matrix from its arguments
    (np.array of longdouble entries stays longdouble; parameters enter as their float64 values, so that 1.0 / c and the like are
    the oracle's); restated where it rounds them into a float64 array (Pleiades, Lorenz-96)."""
    if vf.name == "pleiades":
        return pleiades_jac_ld(u)
    if vf.name == "lorenz96":
        return lorenz96_jac_ld(u)
    J = np.asarray(vf.jac(u, p, t))
    assert J.dtype == np.longdouble or vf.name == "linear", (vf.name, J.dtype)  # linear: the constant diag(p), exact in float64
    return J.astype(np.longdouble)


def filter_ld(vf, u0, q, dt, nsteps, kind="EK1", with_smoother=False, diffusion="dynamic", tgrid=None, full=False, t0=None,
              linearize_at=None):
    """Any oracle vector field (`vf.f` is written for any scalar type, the Jacobian comes from jac_ld; the parameters are handed
    over as their float64 values).  EK0 / EK1 filter and, if asked, the RTS pass (src/smoothing.jl:4-63) over the same records,
    all in longdouble.  diffusion = "dynamic" (src/diffusions.jl:72-80), or "fixed" (src/diffusions.jl:11-36 in the static order of
    src/perform_step.jl:56-63: the filter runs with sigma^2 = 1, the global diffusion is the running mean of z' S^-1 z / d, and the
    postamble, src/integrator_utils.jl:4-18, rescales every covariance by the final one, which is also the diffusion of every
    step of the RTS pass).  tgrid: the save times (float64; step n is the float64 difference tgrid[n+1] - tgrid[n], as on every
    other side); without it nsteps steps of dt.  Returns float64 copies: (means, covs) or (means, covs, smoothed means, smoothed
    covs, diffusions); full=True: a dict of those and the log-likelihood sum -(z' S^-1 z + log det S + d log 2 pi) / 2
    (src/perform_step.jl:66; NaN for "fixed", src/integrator_utils.jl:6).

    The other diffusion models (make_exact.py --models):
      "fixedMAP"   the static order of "fixed" with the on-line mode of the InverseGamma(1/2, 1/2) posterior in place of the running
                   mean (src/diffusions.jl:46-68 as the oracle's perform_step writes it, n_obs = n + 1); log-likelihood NaN.
      "dynamicMV"  EK0; sigma_a = max(z_a^2 / (H Q H')_00, eps_float64), Sigma^- = A X A' + D^1/2 Q D^1/2 with
                   D = kron(I_{q+1}, diag sigma) (src/diffusions.jl:83-112; tests/_mv_reference.py apply_diffusion on the covariance
                   instead of the factor); the log-likelihood is accumulated.
      "fixedMV"    EK0; predicts with the unscaled Q, local_a = z_a^2 / S_00 -- the FIRST diagonal entry of S for every component,
                   as the reference (src/diffusions.jl:115-153) --, running mean per component; the postamble rescales every
                   covariance to D^1/2 Sigma D^1/2 with the final vector; log-likelihood NaN.
    With an MV model the diffusions are [nsteps, d] and the RTS pass uses D^1/2 Q D^1/2 of the step.
    t0: the absolute start time of a field f(u, p, t) (needs tgrid, whose first entry it is): the step evaluates f and the Jacobian
    at tgrid[n + 1] as longdouble, and the Taylor-mode initialisation hands f the jet [t0, 1, 0, ...] (the longdouble twin of
    tests/_time_reference.py time_field).  Without it every evaluation gets t = 0.0, as before.
    linearize_at [n_t, d] float64: the EK1 Jacobian of the step ending at tgrid[k] is evaluated at linearize_at[k] (one IEKS
    iteration, tests/_ieks_reference.py); the residual keeps f(u_pred)."""
    ld = np.longdouble
    d, NB = vf.d, q + 1
    D = d * NB
    p = vf.p
    mv = diffusion in ("dynamicMV", "fixedMV")
    assert diffusion in ("dynamic", "fixed", "fixedMAP", "dynamicMV", "fixedMV"), diffusion
    assert not mv or kind == "EK0", "the MV diffusion models require EK0"
    assert linearize_at is None or kind == "EK1"
    if t0 is not None:
        assert tgrid is not None and float(tgrid[0]) == float(t0)
        tjet = np.zeros(NB, dtype=ld)
        tjet[0] = ld(t0)
        if NB > 1:
            tjet[1] = 1
        t_init = JetLD(tjet)
    else:
        t_init = 0.0
    coef = np.zeros((d, NB), dtype=ld)
    coef[:, 0] = np.asarray(u0, dtype=ld)
    for k in range(q):  # Taylor-mode initial state (src/state_initialization.jl:15-42) in longdouble
        fu = vf.f([JetLD(coef[i].copy()) for i in range(d)], p, t_init)
        for i in range(d):
            coef[i, k + 1] = JetLD.lift(fu[i], NB).c[k] / (k + 1)
    m = np.concatenate([coef[:, k] * ld(math.factorial(k)) for k in range(NB)])
    A = np.eye(D, dtype=ld)
    for i in range(1, q + 1):
        for j in range(d * (q + 1 - i)):
            A[j, j + d * i] = ld(1) / ld(math.factorial(i))
    Q = np.zeros((D, D), dtype=ld)
    for col in range(NB):
        for row in range(NB):
            v = ld(1) / (ld(2 * q + 1 - row - col) * ld(math.factorial(q - row)) * ld(math.factorial(q - col)))
            for i in range(d):
                Q[row * d + i, col * d + i] = v

    def precond(h):
        return np.repeat(np.array([h ** (ld(j) - ld(q) - ld(0.5)) for j in range(NB)], dtype=ld), d)

    if tgrid is None:
        hs = [ld(dt)] * nsteps
    else:
        assert len(tgrid) == nsteps + 1
        hs = [ld(x) for x in np.diff(np.asarray(tgrid, np.float64))]
    Ps = {}
    for h in hs:
        if float(h) not in Ps:
            Ps[float(h)] = precond(h)
    def scaled_q(s2):
        """sigma^2 Q, or D^1/2 Q D^1/2 for a vector of d diffusions."""
        if np.ndim(s2) == 0:
            return s2 * Q
        r = np.tile(np.sqrt(np.asarray(s2, dtype=ld)), NB)
        return np.outer(r, r) * Q

    static = diffusion in ("fixed", "fixedMAP", "fixedMV")
    S_ = np.zeros((D, D), dtype=ld)
    means, covs, diffs = [m.copy()], [S_.copy()], []
    loglik, gdiff = ld(0), None
    for n in range(nsteps):
        P = Ps[float(hs[n])]
        PI = ld(1) / P
        tn = 0.0 if t0 is None else ld(np.float64(tgrid[n + 1]))
        mt, X = P * m, S_ * np.outer(P, P)
        mp_ = A @ mt
        up = (PI * mp_)[:d]
        du = np.asarray(vf.f(list(up), p, tn), dtype=ld)
        z = (PI * mp_)[d:2 * d] - du
        H = np.zeros((d, D), dtype=ld)
        if kind == "EK1":
            ulin = up if linearize_at is None else np.asarray(linearize_at[n + 1], dtype=np.float64).astype(ld)
            H[:, :d] = -jac_ld(vf, ulin, p, tn) * PI[:d][None, :]
        H[:, d:2 * d] = np.diag(PI[d:2 * d])
        if diffusion == "dynamic":
            W = H @ Q @ H.T
            s2 = (z @ solve_spd_ld(W, z[:, None])[:, 0]) / d
            Xp = A @ X @ A.T + s2 * Q
        elif diffusion == "dynamicMV":
            s2 = np.maximum(z * z / (H @ Q @ H.T)[0, 0], ld(np.finfo(np.float64).eps))
            Xp = A @ X @ A.T + scaled_q(s2)
        else:
            Xp = A @ X @ A.T + Q
        C = Xp @ H.T
        Sm = H @ C
        K = solve_spd_ld(Sm, C.T).T
        if diffusion in ("fixed", "fixedMAP"):  # oracle perform_step: success_iter = number of accepted steps so far
            dtn = (z @ solve_spd_ld(Sm, z[:, None])[:, 0]) / d
            if diffusion == "fixed":
                gdiff = dtn if n == 0 else gdiff + (dtn - gdiff) / n
            else:  # mode of the InverseGamma(1/2, 1/2) posterior, on-line (oracle/odefilter_oracle.py perform_step)
                n_obs, alpha, beta, half = n + 1, ld(0.5), ld(0.5), ld(0.5)
                if n == 0:
                    gdiff = (beta + half * dtn) / (alpha + ld(n_obs * d) / 2 + 1)
                else:
                    res_prev = (gdiff * (alpha + ld((n_obs - 1) * d) / 2 + 1) - beta) * 2
                    gdiff = (beta + half * (res_prev + dtn)) / (alpha + ld(n_obs * d) / 2 + 1)
            s2 = gdiff
        elif diffusion == "fixedMV":
            local = z * z / Sm[0, 0]
            gdiff = local if n == 0 else gdiff + (local - gdiff) / n
            s2 = gdiff
        elif full:
            Lc = chol_ld(Sm)
            loglik += -(z @ solve_spd_ld(Sm, z[:, None])[:, 0] + 2 * np.sum(np.log(np.diag(Lc))) + d * np.log(2 * ld(np.pi))) / 2
        mf = mp_ - K @ z
        IKH = np.eye(D, dtype=ld) - K @ H
        Xf = IKH @ Xp @ IKH.T  # Joseph form (see lorenz_mp)
        Xf = (Xf + Xf.T) / 2
        m, S_ = PI * mf, Xf * np.outer(PI, PI)
        means.append(m.copy()); covs.append(S_.copy()); diffs.append(s2)
    if static:  # postamble
        if diffusion == "fixedMV":
            r = np.tile(np.sqrt(gdiff), NB)
            covs = [c * np.outer(r, r) for c in covs]
        else:
            covs = [c * gdiff for c in covs]
        diffs = [gdiff for _ in diffs]
        loglik = ld(np.nan)
    f64 = lambda a: np.array(a).astype(np.float64)  # noqa: E731
    if not with_smoother:
        return f64(means), f64(covs)
    # RTS pass: x_i^s from x_i (filter) and x_{i+1}^s, G = X A' (A X A' + sigma_i^2 Q)^-1 in preconditioned coordinates;
    # diffusions[i] belongs to the step t_i -> t_{i+1} (src/integrator_utils.jl:44)
    sm, sc = [None] * (nsteps + 1), [None] * (nsteps + 1)
    sm[nsteps], sc[nsteps] = means[nsteps], covs[nsteps]
    sm[0], sc[0] = means[0], covs[0]
    for i in range(nsteps - 1, 0, -1):
        P = Ps[float(hs[i])]
        PI = ld(1) / P
        PP = np.outer(P, P)
        mt, X = P * means[i], covs[i] * PP
        B = A @ X @ A.T + scaled_q(diffs[i])
        B = (B + B.T) / 2
        G = solve_spd_ld(B, A @ X).T  # X A' B^-1 (X, B symmetric)
        ms_ = mt + G @ (P * sm[i + 1] - A @ mt)
        Ss = X + G @ (sc[i + 1] * PP - B) @ G.T
        Ss = (Ss + Ss.T) / 2
        sm[i], sc[i] = PI * ms_, Ss * np.outer(PI, PI)
    if full:
        return dict(mean_filt=f64(means), cov_filt=f64(covs), mean_smooth=f64(sm), cov_smooth=f64(sc), diffusions=f64(diffs),
                    loglik=float(loglik))
    return f64(means), f64(covs), f64(sm), f64(sc), f64(diffs)


def team_fixture(vf, u0s, trajs, q, kind, nsteps, dt, with_loglik=False):
    """Trajectories `trajs` of the ensemble `u0s`: filter and smoother in extended precision, and the float64 oracle's distance
    from them -- per derivative block for the means (all records) and for the covariance at one record each: the LAST filter
    record and smoothed record 1 (the one the backward pass reaches last), stored as packed lower triangles."""
    d = vf.d
    D = d * (q + 1)
    il = np.tril_indices(D)
    out = dict(trajs=np.array(trajs), u0s=u0s[list(trajs)], dt=dt, nsteps=nsteps, order=q, ek1=int(kind == "EK1"),
               cov_record_filt=nsteps, cov_record_smooth=1)
    acc = {k: [] for k in ("mean_filt", "mean_smooth", "diffusions", "cov_filt_tril", "cov_smooth_tril", "oracle_block_err_filt",
                           "oracle_block_err_smooth", "oracle_cov_err_filt", "oracle_cov_err_smooth", "oracle_diffusion_err")}
    if with_loglik:
        acc["loglik"], acc["oracle_loglik_err"] = [], []
    for i in trajs:
        r = filter_ld(vf, u0s[i], q, dt, nsteps, kind=kind, with_smoother=True, full=True)
        mf, cf, ms, cs, df = r["mean_filt"], r["cov_filt"], r["mean_smooth"], r["cov_smooth"], r["diffusions"]
        sol = orc.solve(vf, orc.Alg(kind, q, "dynamic", True), u0=u0s[i], tspan=(0.0, nsteps * dt), dt=dt)
        acc["mean_filt"].append(mf); acc["mean_smooth"].append(ms); acc["diffusions"].append(df)
        acc["cov_filt_tril"].append(cf[nsteps][il]); acc["cov_smooth_tril"].append(cs[1][il])
        acc["oracle_block_err_filt"].append(block_err(sol.means(smoothed=False), mf, d))
        acc["oracle_block_err_smooth"].append(block_err(sol.means(smoothed=True), ms, d))
        acc["oracle_cov_err_filt"].append(cov_err(sol.covs(smoothed=False)[nsteps:nsteps + 1], cf[nsteps:nsteps + 1]))
        acc["oracle_cov_err_smooth"].append(cov_err(sol.covs(smoothed=True)[1:2], cs[1:2]))
        acc["oracle_diffusion_err"].append(float(np.max(np.abs(sol.diffusions - df) / np.abs(df))))
        if with_loglik:
            acc["loglik"].append(r["loglik"])
            acc["oracle_loglik_err"].append(abs(sol.log_likelihood - r["loglik"]) / abs(r["loglik"]))
    out.update({k: np.array(v) for k, v in acc.items()})
    return out


def pleiades_fixture(q, kind, nsteps, dt, trajs=(0, 4)):
    """Trajectories `trajs` of the Pleiades ensemble (positions perturbed by 1e-3), see team_fixture."""
    vp = orc.vector_field("pleiades")
    return team_fixture(vp, orc.ensemble_u0(vp.u0, max(trajs) + 1, 1e-3, n_perturbed=14), trajs, q, kind, nsteps, dt)


def lorenz96_fixture(q, kind, nsteps=12, dt=2.0**-7, trajs=(0, 5)):
    vf = orc.vector_field("lorenz96")
    return team_fixture(vf, orc.ensemble_u0(vf.u0, 6, 1e-2), trajs, q, kind, nsteps, dt, with_loglik=True)


ADMIT_DIFFUSION_ERR = 1e-4  # see the module docstring


def small_fixture(rhs, kind, q, diffusion, dt, nsteps=SMALL_NSTEPS, ntraj=SMALL_NTRAJ):
    """Trajectories 0 ... ntraj-1 of ensemble_u0(u0, ntraj, 1e-2) on the save times np.arange(nsteps + 1) * dt: filter and
    smoother in extended precision with the covariances of EVERY record (packed lower triangles), the diffusions and the
    log-likelihood; next to them the float64 oracle's distance from each, per trajectory."""
    vf = orc.vector_field(rhs)
    u0s = orc.ensemble_u0(vf.u0, ntraj, 1e-2)
    tg = np.arange(nsteps + 1) * dt
    D = vf.d * (q + 1)
    il = np.tril_indices(D)
    out = dict(rhs=rhs, kind=kind, order=q, ek1=int(kind == "EK1"), diffusionmodel=diffusion, dt=dt, nsteps=nsteps, t=tg,
               trajs=np.arange(ntraj), u0s=u0s)
    acc = {k: [] for k in ("mean_filt", "mean_smooth", "cov_filt_tril", "cov_smooth_tril", "diffusions", "loglik",
                           "oracle_block_err_filt", "oracle_block_err_smooth", "oracle_cov_err_filt", "oracle_cov_err_smooth",
                           "oracle_diffusion_err", "oracle_loglik_err")}
    for i in range(ntraj):
        r = filter_ld(vf, u0s[i], q, dt, nsteps, kind=kind, with_smoother=True, diffusion=diffusion, tgrid=tg, full=True)
        sol = orc.solve(vf, orc.Alg(kind, q, diffusion, True), u0=u0s[i], tgrid=tg)
        assert len(sol.t) == nsteps + 1 and sol.retcode == "Success"
        for name, sm in (("filt", False), ("smooth", True)):
            acc["mean_" + name].append(r["mean_" + name])
            acc[f"cov_{name}_tril"].append(r["cov_" + name][:, il[0], il[1]])
            acc["oracle_block_err_" + name].append(block_err(sol.means(smoothed=sm), r["mean_" + name], vf.d))
            acc["oracle_cov_err_" + name].append(cov_err(sol.covs(smoothed=sm)[1:], r["cov_" + name][1:]))  # record 0: zero
        acc["diffusions"].append(r["diffusions"]); acc["loglik"].append(r["loglik"])
        acc["oracle_diffusion_err"].append(float(np.max(np.abs(np.asarray(sol.diffusions) - r["diffusions"]) / np.abs(r["diffusions"]))))
        acc["oracle_loglik_err"].append(abs(sol.log_likelihood - r["loglik"]) / abs(r["loglik"]) if diffusion == "dynamic" else np.nan)
    out.update({k: np.array(v) for k, v in acc.items()})
    return out


def model_fixture(case, nsteps=SMALL_NSTEPS, ntraj=SMALL_NTRAJ):
    """A MODEL_CASES fixture in the layout of small_fixture.  The float64 side of the yardstick: orc.solve ("map", "forced"),
    tests/_mv_reference.py solve ("mv"), tests/_ieks_reference.py solve_ieks running its own chain of IEKS_ITERATIONS iterations
    ("ieks"; the extended-precision chain linearises iteration j at the float64 rounding of its own iteration j - 1's smoothed u,
    as a device reads it back from a float64 record)."""
    family, rhs, kind, q, diffusion, dt = case
    vf = X.model_field(case)
    u0s = orc.ensemble_u0(vf.u0, ntraj, 1e-2)
    tg = X.model_grid(case)[: nsteps + 1]
    t0 = X.MODEL_T0 if family == "forced" else None
    d = vf.d
    il = np.tril_indices(d * (q + 1))
    with_loglik = diffusion in ("dynamic", "dynamicMV")
    out = dict(family=family, rhs=rhs, kind=kind, order=q, ek1=int(kind == "EK1"), diffusionmodel=diffusion, dt=dt, nsteps=nsteps, t=tg,
               trajs=np.arange(ntraj), u0s=u0s)
    if family == "ieks":
        out["iterations"] = X.IEKS_ITERATIONS
    acc = {k: [] for k in ("mean_filt", "mean_smooth", "cov_filt_tril", "cov_smooth_tril", "diffusions", "loglik",
                           "oracle_block_err_filt", "oracle_block_err_smooth", "oracle_cov_err_filt", "oracle_cov_err_smooth",
                           "oracle_diffusion_err", "oracle_loglik_err")}
    for i in range(ntraj):
        kw = dict(kind=kind, with_smoother=True, diffusion=diffusion, tgrid=tg, full=True, t0=t0)
        if family == "ieks":
            lin = None
            for _ in range(X.IEKS_ITERATIONS):
                r = filter_ld(vf, u0s[i], q, dt, nsteps, linearize_at=lin, **kw)
                lin = r["mean_smooth"][:, :d]
            sol = ier.solve_ieks(vf, q, diffusion, tg, X.IEKS_ITERATIONS, u0=u0s[i])
        else:
            r = filter_ld(vf, u0s[i], q, dt, nsteps, **kw)
            if family == "mv":
                sol = mvr.solve(vf, diffusion, q, u0=u0s[i], tspan=(tg[0], tg[-1]), tgrid=tg)
            else:
                sol = orc.solve(vf, orc.Alg(kind, q, diffusion, True), u0=u0s[i], tspan=(tg[0], tg[-1]), tgrid=tg)
        assert len(sol.t) == nsteps + 1 and sol.retcode == "Success"
        for name, sm in (("filt", False), ("smooth", True)):
            acc["mean_" + name].append(r["mean_" + name])
            acc[f"cov_{name}_tril"].append(r["cov_" + name][:, il[0], il[1]])
            acc["oracle_block_err_" + name].append(block_err(sol.means(smoothed=sm), r["mean_" + name], d))
            acc["oracle_cov_err_" + name].append(cov_err(sol.covs(smoothed=sm)[1:], r["cov_" + name][1:]))  # record 0: zero
        acc["diffusions"].append(r["diffusions"]); acc["loglik"].append(r["loglik"])
        od = np.asarray(sol.diffusions, float)
        assert od.shape == r["diffusions"].shape, (od.shape, r["diffusions"].shape)
        acc["oracle_diffusion_err"].append(float(np.max(np.abs(od - r["diffusions"]) / np.abs(r["diffusions"]))))  # MV: per component
        acc["oracle_loglik_err"].append(abs(sol.log_likelihood - r["loglik"]) / abs(r["loglik"]) if with_loglik else np.nan)
    out.update({k: np.array(v) for k, v in acc.items()})
    return out


def admit(name, fx):
    worst = float(np.max(fx["oracle_diffusion_err"]))
    assert worst <= ADMIT_DIFFUSION_ERR, (f"{name}: the oracle's diffusions are {worst:.1e} relative off the extended-precision ones "
                                          f"(> {ADMIT_DIFFUSION_ERR}): rounding noise, no yardstick -- pick another step size")


def write_if_changed(path, fx):
    """Leave a committed fixture alone when its contents are what was just computed."""
    if os.path.exists(path):
        old = np.load(path)
        if sorted(old.files) == sorted(fx) and all(np.array_equal(old[k], np.asarray(fx[k]), equal_nan=np.asarray(fx[k]).dtype.kind == "f") for k in fx):
            return False
    np.savez_compressed(path, **fx)
    return True


def main_small():
    for rhs, kind, q, diffusion, dt in SMALL_CASES:
        name = small_name(rhs, kind, q, diffusion)
        fx = small_fixture(rhs, kind, q, diffusion, dt)
        admit(name, fx)
        wrote = write_if_changed(os.path.join(HERE, name + ".npz"), fx)
        print(name, "(written)" if wrote else "(unchanged)", ": oracle vs extended precision, filter blocks", fx["oracle_block_err_filt"].max(axis=0),
              "cov", fx["oracle_cov_err_filt"].max(), "| smoother blocks", fx["oracle_block_err_smooth"].max(axis=0), "cov",
              fx["oracle_cov_err_smooth"].max(), "| diffusions", fx["oracle_diffusion_err"].max(), "loglik", fx["oracle_loglik_err"].max(), flush=True)
    for kind, q in LORENZ96_CASES:
        name = lorenz96_name(kind, q)
        fx = lorenz96_fixture(q, kind)
        admit(name, fx)
        wrote = write_if_changed(os.path.join(HERE, name + ".npz"), fx)
        print(name, "(written)" if wrote else "(unchanged)", ": oracle vs extended precision, filter blocks", fx["oracle_block_err_filt"].max(axis=0),
              "cov", fx["oracle_cov_err_filt"], "| smoother blocks", fx["oracle_block_err_smooth"].max(axis=0), "cov", fx["oracle_cov_err_smooth"],
              "| diffusions", fx["oracle_diffusion_err"], "loglik", fx["oracle_loglik_err"], flush=True)


def main_models(cases=None):
    for case in (X.MODEL_CASES if cases is None else cases):
        name = X.model_name(case)
        fx = model_fixture(case)
        admit(name, fx)
        wrote = write_if_changed(os.path.join(HERE, name + ".npz"), fx)
        print(name, "(written)" if wrote else "(unchanged)", ": oracle vs extended precision, filter blocks", fx["oracle_block_err_filt"].max(axis=0),
              "cov", fx["oracle_cov_err_filt"].max(), "| smoother blocks", fx["oracle_block_err_smooth"].max(axis=0), "cov",
              fx["oracle_cov_err_smooth"].max(), "| diffusions", fx["oracle_diffusion_err"].max(), "loglik", np.nanmax(fx["oracle_loglik_err"])
              if np.isfinite(fx["oracle_loglik_err"]).any() else np.nan, flush=True)


if __name__ == "__main__":
    if "--small" in sys.argv[1:]:
        main_small()
        sys.exit(0)
    if "--models" in sys.argv[1:]:
        main_models()
        sys.exit(0)
    vf = orc.vector_field("lorenz63")
    u0 = orc.ensemble_u0(vf.u0, 1, 1e-2)[0]
    dt, ns = 2.0**-9, 1024
    mf, cf, ms, cs, df = lorenz_mp(u0, vf.p, 3, dt, ns)
    sol = orc.solve(vf, orc.EK1(order=3, smooth=True), u0=u0, tspan=(0.0, ns * dt), dt=dt)
    out = dict(u0=u0, dt=dt, nsteps=ns, digits=50, mean_filt=mf, cov_filt=cf, mean_smooth=ms, cov_smooth=cs, diffusions=df,
               oracle_block_err_filt=block_err(sol.means(smoothed=False), mf, 3), oracle_cov_err_filt=cov_err(sol.covs(smoothed=False), cf),
               oracle_block_err_smooth=block_err(sol.means(smoothed=True), ms, 3), oracle_cov_err_smooth=cov_err(sol.covs(smoothed=True), cs))
    np.savez_compressed(os.path.join(HERE, "exact_lorenz_mp.npz"), **out)
    print("exact_lorenz_mp: oracle vs exact, filter blocks", out["oracle_block_err_filt"], "cov", out["oracle_cov_err_filt"],
          "| smoother blocks", out["oracle_block_err_smooth"], "cov", out["oracle_cov_err_smooth"])

    vp = orc.vector_field("pleiades")
    u0p = orc.ensemble_u0(vp.u0, 1, 1e-3, n_perturbed=14)[0]
    dtp, nsp = 2.0**-10, 24
    mfp, cfp = filter_ld(vp, u0p, 5, dtp, nsp)
    solp = orc.solve(vp, orc.EK1(order=5, smooth=False), u0=u0p, tspan=(0.0, nsp * dtp), dt=dtp)
    outp = dict(u0=u0p, dt=dtp, nsteps=nsp, mean_filt=mfp, var_filt=np.array([np.diag(c) for c in cfp]), cov_final=cfp[-1],
                oracle_block_err_filt=block_err(solp.means(smoothed=False), mfp, 28),
                oracle_cov_err_final=cov_err(solp.covs(smoothed=False)[-1:], cfp[-1:]))
    np.savez_compressed(os.path.join(HERE, "exact_pleiades_ld.npz"), **outp)
    print("exact_pleiades_ld: oracle vs extended precision, filter blocks", outp["oracle_block_err_filt"], "final cov", outp["oracle_cov_err_final"])

    # filter + smoother at the sizes of the GPU parity tests (tests/test_gpu_parity.py test_pleiades_ensemble_parity: 12 steps of
    # config 4's dt = 2^-10), and order 5 once more with dt = 2^-6: at 2^-10 the residuals of the first steps of an order-5 solve are
    # h^5-small, i.e. rounding noise in float64 (the oracle's own diffusions are 40 % off there) -- the larger step is where
    # an order-5 covariance can be checked sharply
    for q_, kind_, dt_, tag in ((2, "EK1", 2.0**-10, ""), (3, "EK0", 2.0**-10, ""), (5, "EK1", 2.0**-10, ""), (5, "EK1", 2.0**-6, "_dt6")):
        fxp = pleiades_fixture(q_, kind_, 12, dt_)
        name = f"exact_pleiades_{kind_.lower()}q{q_}{tag}_smooth_ld"
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **fxp)
        print(name, ": oracle vs extended precision, filter blocks", fxp["oracle_block_err_filt"].max(axis=0), "cov", fxp["oracle_cov_err_filt"],
              "| smoother blocks", fxp["oracle_block_err_smooth"].max(axis=0), "cov", fxp["oracle_cov_err_smooth"], "| diffusions", fxp["oracle_diffusion_err"])
