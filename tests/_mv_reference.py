"""numpy restatement of the diagonal ("multivariate") diffusion models :dynamicMV / :fixedMV of EK0
(src/diffusions.jl:83-153), built from the oracle's pieces.

A diffusion here is a vector sigma[d]: Sigma = diag(sigma), applied to the process noise as
apply_diffusion(Q, Diagonal) = X_A_Xt(Q, sqrt.(kron(I_{q+1}, Sigma))) (src/ProbNumDiffEq.jl:38) -- on the square-root
factor Q_L that is a row scaling by sqrt(sigma_a) of every row (J, a).  Step orders (src/perform_step.jl:40-63):
:dynamicMV calibrates, then predicts with the scaled Q; :fixedMV predicts with the unscaled Q, measures, then
calibrates, and the postamble (src/integrator_utils.jl:4-18) rescales every filter covariance to
sqrt(D) Sigma sqrt(D), D = kron(I, sigma_final).  The smoother, dense output and sampler are the oracle's with the
diagonal diffusion of the step (src/smoothing.jl:21, src/solution.jl:181-205, src/solution_sampling.jl:42-45).
"""
import math

import numpy as np

import odefilter_oracle as orc

MV_MODELS = ("dynamicMV", "fixedMV")
EPS = float(np.finfo(float).eps)


def apply_diffusion(Q_L: np.ndarray, sigma, q: int) -> np.ndarray:
    """SR form of X_A_Xt(Q, sqrt.(kron(I_{q+1}, Diagonal(sigma)))): rows (J, a) of Q_L times sqrt(sigma_a)."""
    return np.tile(np.sqrt(np.asarray(sigma, float)), q + 1)[:, None] * Q_L


def perform_step(model: str, vf, p, consts, x: orc.SRGaussian, t: float, dt: float, success_iter: int = 0,
                 prev_global=None) -> orc.StepResult:
    """src/perform_step.jl:27-76 with an MV diffusion model, EK0 (H = E1 PI, src/diffusions.jl:96, :125)."""
    A, Q_L, precond, d, q = consts
    alg = orc.EK0(order=q)
    P = precond(dt)
    PI = 1.0 / P
    xp = orc.linmap(P, x)
    m_pred = orc.predict_mean(xp.mu, A)
    z, H, _ = orc.measure(alg, vf, p, m_pred, PI, t + dt, d, q)
    if model == "dynamicMV":  # src/diffusions.jl:83-112
        HQ = H @ Q_L
        q0_11 = (HQ @ HQ.T)[0, 0]
        sigma = np.maximum(z**2 / q0_11, EPS)
        local = glob = sigma
        L_pred, used_qr = orc.predict_cov_sr(xp.L, A, apply_diffusion(Q_L, sigma, q))
        HL = H @ L_pred
        S = HL @ HL.T
    elif model == "fixedMV":  # src/diffusions.jl:115-153
        L_pred, used_qr = orc.predict_cov_sr(xp.L, A, Q_L)
        HL = H @ L_pred
        S = HL @ HL.T
        local = z**2 / S[0, 0]  # the FIRST diagonal entry of S for every component, as the reference
        glob = local if success_iter == 0 else prev_global + (local - prev_global) / success_iter
    else:
        raise ValueError(model)
    x_pred = orc.SRGaussian(m_pred, L_pred)
    ll = orc.logpdf_zero(z, S)
    x_filt = orc.update(x_pred, z, S, H)
    return orc.StepResult(x_filt=orc.linmap(PI, x_filt), x_pred=orc.linmap(PI, x_pred), x_back=orc.linmap(PI, xp),
                          u_filt=(PI * x_filt.mu)[:d], local_diffusion=local, global_diffusion=glob, log_likelihood=ll,
                          H=H, z=z, S=S, used_qr=used_qr)


def estimate_errors(local, Q_L: np.ndarray, H: np.ndarray, q: int) -> np.ndarray:
    """src/perform_step.jl:148-158: err_r = sqrt(diag(H (sigma Q) H'))_r."""
    HQ = H @ apply_diffusion(Q_L, local, q)
    return np.sqrt(np.diag(HQ @ HQ.T))


def solve(vf, model: str, order: int, *, u0=None, p=None, tspan=None, dt=None, adaptive=False, abstol=1e-6,
          reltol=1e-3, smooth=True, tgrid=None, maxiters=100000) -> orc.Solution:
    """orc.solve with an MV diffusion model: same loop, same controller, `sol.diffusions` a list of d-vectors."""
    u0 = vf.u0 if u0 is None else np.asarray(u0, float)
    p = vf.p if p is None else np.asarray(p, float)
    tspan = vf.tspan if tspan is None else tspan
    d, q = len(u0), order
    consts = orc.make_consts(d, q)
    t0, t1 = tspan
    x = orc.initial_update(u0, vf, p, t0, q)
    sol = orc.Solution(d=d, q=q)
    sol.t.append(t0)
    sol.x_filt.append(x.copy())
    u_cur = np.asarray(u0, float).copy()
    if not adaptive:
        grid = orc.fixed_time_grid(t0, t1, dt) if tgrid is None else np.asarray(tgrid, float)
        for n in range(len(grid) - 1):
            prev = sol.diffusions[-1] if sol.diffusions else None
            res = perform_step(model, vf, p, consts, x, grid[n], grid[n + 1] - grid[n], sol.naccept, prev)
            sol.nf += 1
            x = res.x_filt
            sol.log_likelihood += res.log_likelihood
            sol.naccept += 1
            sol.t.append(grid[n + 1])
            sol.x_filt.append(x.copy())
            sol.diffusions.append(res.global_diffusion)
    else:
        ctrl = orc.Controller.default(q)
        t, h = t0, (dt if dt is not None else 1e-3)
        qold, q11, iters = ctrl.qoldinit, 1.0, 0
        while t < t1:
            iters += 1
            if iters > maxiters:
                sol.retcode = "MaxIters"
                break
            h = min(h, t1 - t)
            prev = sol.diffusions[-1] if sol.diffusions else None
            res = perform_step(model, vf, p, consts, x, t, h, sol.naccept, prev)
            sol.nf += 1
            e = estimate_errors(res.local_diffusion, consts[1], res.H, q)
            err = h * e / (abstol + np.maximum(np.abs(u_cur), np.abs(res.u_filt)) * reltol)
            EEst = orc.internalnorm(err)
            u_cur = res.u_filt
            if not math.isfinite(EEst):
                EEst = float("inf")
            if EEst == 0.0:
                qq = 1.0 / ctrl.qmax
            else:
                q11 = EEst**ctrl.beta1
                qq = max(1.0 / ctrl.qmax, min(1.0 / ctrl.qmin, q11 / (qold**ctrl.beta2) / ctrl.gamma))
            if EEst <= 1.0:
                if EEst < 1.0:
                    x = res.x_filt
                    sol.log_likelihood += res.log_likelihood
                else:
                    x = res.x_back
                if ctrl.qsteady_min <= qq <= ctrl.qsteady_max:
                    qq = 1.0
                qold = max(EEst, ctrl.qoldinit)
                tn = t + h
                if abs(tn - t1) < 100 * EPS * max(abs(tn), abs(t1)):
                    tn = t1
                t = tn
                sol.naccept += 1
                sol.t.append(t)
                sol.x_filt.append(x.copy())
                sol.diffusions.append(res.global_diffusion)
                h = h / qq
            else:
                x = res.x_back
                sol.nreject += 1
                h = h / min(1.0 / ctrl.qmin, q11 / ctrl.gamma)
    if model == "fixedMV" and sol.diffusions:  # postamble! (src/integrator_utils.jl:4-18)
        final = sol.diffusions[-1]
        sol.log_likelihood = float("nan")
        sq = np.tile(np.sqrt(final), q + 1)
        for s in sol.x_filt:
            s.L = sq[:, None] * s.L  # sqrt(D) Sigma sqrt(D)
        sol.diffusions = [final.copy() for _ in sol.diffusions]
    if smooth:
        smooth_all(sol, consts)
    return sol


def smooth_all(sol: orc.Solution, consts) -> None:
    """src/smoothing.jl:4-28 with Qh = apply_diffusion(Q, diffusions[i])."""
    A, Q_L, precond, d, q = consts
    x = [g.copy() for g in sol.x_filt]
    t = sol.t
    for i in range(len(x) - 2, 0, -1):
        h = t[i + 1] - t[i]
        if h == 0:
            x[i] = x[i + 1].copy()
            continue
        P = precond(h)
        xs, _ = orc.smooth(orc.linmap(P, x[i]), orc.linmap(P, x[i + 1]), A, apply_diffusion(Q_L, sol.diffusions[i], q))
        x[i] = orc.linmap(1.0 / P, xs)
    sol.x_smooth = x


def dense_output(sol: orc.Solution, consts, tval: float, smoothed: bool = True) -> orc.SRGaussian:
    """src/solution.jl:165-210 with the diagonal diffusion of the interval."""
    A, Q_L, precond, d, q = consts
    t = np.asarray(sol.t)
    idx = int(np.sum(t <= tval))
    if np.any(t == tval):
        return (sol.x_smooth if smoothed else sol.x_filt)[idx - 1]
    Qh = apply_diffusion(Q_L, sol.diffusions[min(idx, len(sol.diffusions)) - 1], q)
    P = precond(tval - t[idx - 1])
    goal_pred = orc.linmap(1.0 / P, orc.predict(orc.linmap(P, sol.x_filt[idx - 1]), A, Qh))
    if not smoothed or tval >= t[-1]:
        return goal_pred
    P = precond(t[idx] - tval)
    gs, _ = orc.smooth(orc.linmap(P, goal_pred), orc.linmap(P, sol.x_smooth[idx]), A, Qh)
    return orc.linmap(1.0 / P, gs)


def sample_states(sol: orc.Solution, consts, n: int = 1, seed: int = 0x5A3B1E, traj: int = 0, noise_scale: float = 1.0,
                  n_save=None) -> np.ndarray:
    """src/solution_sampling.jl:24-62 on the saved grid with the diagonal diffusions, the device's square root (the
    lower Cholesky factor) and its noise stream (orc.sample_normal; `n_save`: the save axis of the device's counter).
    Returns [n_save, D, n]."""
    A, Q_L, precond, d, q = consts
    D = d * (q + 1)
    ts, xs = sol.t, sol.x_filt
    ns = len(xs)
    nsc = ns if n_save is None else n_save
    path = np.zeros((ns, D, n))

    def draw(g, j, slot):
        xi = np.array([orc.sample_normal(seed, traj, j, slot, k, n, nsc, D) for k in range(D)])
        return g.mu + noise_scale * (orc.lower_factor(g.L @ g.L.T) @ xi)

    for j in range(n):
        path[ns - 1, :, j] = draw(xs[-1], j, ns - 1)
    for i in range(ns - 2, -1, -1):
        dt = ts[i + 1] - ts[i]
        i_diff = int(np.sum(np.asarray(ts, float) <= ts[i]))
        Qh = apply_diffusion(Q_L, sol.diffusions[i_diff - 1], q)
        P = precond(dt)
        for j in range(n):
            nxt = orc.SRGaussian(P * path[i + 1, :, j], np.zeros((D, D)))
            prev_p, _ = orc.smooth(orc.linmap(P, xs[i]), nxt, A, Qh)
            path[i, :, j] = draw(orc.linmap(1.0 / P, prev_p), j, i)
    return path
