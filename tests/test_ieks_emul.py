"""Host build of the IEKS step (tests/emul/emul_ieks.cpp: ek_filter_fixed_ieks_kernel's lane body with and without lagged
record stores, and ek_filter_rows_ieks_kernel's row-team body) against the numpy restatement of solve_ieks
(tests/_ieks_reference.py), iteration by iteration, with the emulated smoother feeding the next iteration's linearisation
points as odef_smooth does on the device (CPU only)."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import _emul as em
import _ieks_reference as ier
import odefilter_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        src = os.path.join(HERE, "emul", "emul_ieks.cpp")
        out = os.path.join(HERE, "emul", "libodef_emul_ieks.so")
        deps = [src, os.path.join(HERE, "emul", "emul.cpp")] + glob.glob(os.path.join(em.ROOT, "odefilters.jl_amd", "csrc", "*.h"))
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            subprocess.check_call(["g++", "-O1", "-std=c++20", "-shared", "-fPIC", "-Wno-unknown-pragmas", src, "-o", out])
        _LIB = C.CDLL(out)
        _LIB.emul_precond_fill.argtypes = [C.c_int, C.c_double, C.c_double, em.dp]
    return _LIB


def emul_ieks(rhs_id, d, q, u0s, p, grid, model, iterations, kernel, ps=None):
    """solve_ieks on the emulated kernels: [per iteration] (smoothed mean [N, n_t, D], filter mean, loglik, njac).
    ps: parameters per trajectory [N, n_params] in place of the shared p."""
    u0s = np.asarray(u0s, float)
    N, D = u0s.shape[0], d * (q + 1)
    TRI = D * (D + 1) // 2
    At, Qt, QLt = em.prior_tables(q)
    u0_dev = np.ascontiguousarray(u0s.T)
    p = np.ascontiguousarray(np.asarray(p, float) if ps is None else np.asarray(ps, float).T)
    tg = np.ascontiguousarray(np.asarray(grid, float))
    hs = np.ascontiguousarray(np.diff(tg))
    nsteps, n_save = len(hs), len(tg)
    uniq, inv = np.unique(hs, return_inverse=True)
    ptab = np.zeros((len(uniq), lib().emul_tab_stride()))
    for k, h in enumerate(uniq):
        lib().emul_precond_fill(q, float(h), float(h) ** (-q - 1 / 2), em._p(ptab[k]))
    tab_idx = np.ascontiguousarray(inv.astype(np.int32))
    ctrl = np.zeros(10)
    a = em.EmulArgs()
    a.rhs, a.q, a.ek1, a.adaptive = rhs_id, q, 1, 0
    a.N, a.u0, a.p, a.p_shared = N, em._p(u0_dev), em._p(p), int(ps is None)
    a.At, a.Qt, a.QLt = em._p(At), em._p(Qt), em._p(QLt)
    a.hs, a.ptab, a.tab_idx, a.nsteps = em._p(hs), em._p(ptab), em._p(tab_idx, em.ip), nsteps
    a.t0, a.ctrl, a.max_save = float(tg[0]), em._p(ctrl), 0
    a.everystep, a.fixed_diffusion, a.want_loglik = 1, {"dynamic": 0, "fixed": 1, "fixedMAP": 2}[model], 1
    out, lin = [], None
    for _ in range(iterations):
        mean = np.zeros((n_save, D, N)); cov = np.zeros((n_save, TRI, N)); diff = np.zeros((n_save, N))
        tsave = np.zeros((n_save, N)); loglik = np.zeros(N)
        ints = [np.zeros(N, np.int32) for _ in range(6)]
        a.mean, a.cov, a.diff, a.tsave, a.loglik = em._p(mean), em._p(cov), em._p(diff), em._p(tsave), em._p(loglik)
        a.naccept, a.nreject, a.nf, a.njac, a.nsaved, a.retcode = [em._p(x, em.ip) for x in ints]
        if lin is None:  # the empty field: the EK1 kernels, emulated by emul.cpp
            a.everystep = {0: 1, 1: 2, 2: 3}[kernel]
            assert lib().emul_filter(C.byref(a)) == 0
            a.everystep = 1
        else:
            assert lib().emul_filter_ieks(C.byref(a), em._p(lin), kernel) == 0
        if model != "dynamic":  # postamble! (src/integrator_utils.jl:4-18), the device's scale_cov_kernel
            cov *= diff[-1][None, None, :]
            diff[1:] = diff[-1][None, :]
            loglik[:] = np.nan
        smean = np.zeros_like(mean); scov = np.zeros_like(cov)
        a.smean, a.scov, a.n_save = em._p(smean), em._p(scov), n_save
        assert lib().emul_smooth(C.byref(a), d) == 0
        lin = np.ascontiguousarray(smean[:, :d, :])  # odef_smooth: rows 0..d-1 of every SMOOTH_MEAN save
        out.append((smean.transpose(2, 0, 1), mean.transpose(2, 0, 1), loglik.copy(), ints[3].copy()))
    return out


def _rel(a, b):
    return float(np.nanmax(np.abs(a - b)) / np.nanmax(np.abs(b)))


CASES = [("fhn", 0, 4, "fixed", 0.1, (0.0, 6.0)), ("lorenz63", 1, 3, "dynamic", 2.0**-8, (0.0, 1.0)),
         ("vanderpol", 3, 5, "fixedMAP", 0.02, (0.0, 1.0))]


@pytest.mark.parametrize("kernel", [0, 1, 2])
@pytest.mark.parametrize("rhs,rid,q,model,dt,tspan", CASES)
def test_emulated_ieks_kernels_match_restatement(rhs, rid, q, model, dt, tspan, kernel):
    vf = orc.vector_field(rhs)
    d = vf.d
    if kernel == 2 and d * (q + 1) > 16:
        pytest.skip("row-team kernels serve state dimension <= 16")
    grid = orc.fixed_time_grid(tspan[0], tspan[1], dt)
    u0s = np.stack([vf.u0, vf.u0 * 1.01 + 0.01])
    iters = 3
    tol = 1e-9 if q <= 4 else 1e-5  # q = 5: Q is Hilbert-like, the higher derivatives amplify rounding (tests/_parity.py)
    got = emul_ieks(rid, d, q, u0s, vf.p, grid, model, iters, kernel)
    for j, u0 in enumerate(u0s):
        ref = ier.solve_ieks(vf, q, model, grid, iters, u0=u0, history=True)
        for k in range(iters):
            smean, mean, ll, njac = got[k]
            assert _rel(smean[j], ref[k].means(smoothed=True)) < tol, (k, j)
            assert _rel(mean[j], ref[k].means(smoothed=False)) < tol, (k, j)
            assert njac[j] == len(grid) - 1
            if model == "dynamic":
                assert abs(ll[j] - ref[k].log_likelihood) <= 1e-8 * abs(ref[k].log_likelihood)
        # the iterates move: iteration 2 is not EK1
        assert not np.array_equal(got[1][0][j], got[0][0][j])
