"""The wave -> trajectory map of the fixed-step lane filter kernels (csrc/wave_map.h, ODEF_WAVE_MAP).

CPU: the map itself, compiled into a stand-alone host program -- a bijection of the blocks for every grid size, one contiguous
ascending range per residue class mod 8, the ranges in residue order.  GPU (`-m gpu`): a trajectory's arithmetic does not
depend on the wavefront that carries it, so every output of a solve under the XCD-contiguous map must equal the identity map's
bit for bit, on ensembles whose partial wavefront then sits in the middle of the grid."""
import os
import subprocess

import numpy as np
import pytest

import _parity as P
import odefilter_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "odefilters.jl_amd", "csrc")
N_BLOCKS = [1, 2, 7, 8, 9, 15, 16, 17, 1023, 1024, 1025]

_PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "wave_map.h"
int main(int argc, char** argv) {  // wave_map <mode> <n_blocks>...: one line per n_blocks, the first trajectory of every block
  const int mode = atoi(argv[1]);
  for (int k = 2; k < argc; ++k) {
    const unsigned n = (unsigned)atol(argv[k]);
    for (unsigned b = 0; b < n; ++b) printf("%ld ", odef::wave_first_trajectory(b, n, mode));
    printf("\n");
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def wave_map(tmp_path_factory):
    """{mode: {n_blocks: slot of every block}} from the header's own function."""
    tmp = tmp_path_factory.mktemp("wave_map")
    src, exe = tmp / "wave_map_main.cpp", tmp / "wave_map_main"
    src.write_text(_PROGRAM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    out = {}
    for mode in (0, 1):
        lines = subprocess.run([str(exe), str(mode)] + [str(n) for n in N_BLOCKS], check=True, capture_output=True, text=True).stdout
        rows = [np.array(ln.split(), dtype=np.int64) for ln in lines.strip().split("\n")]
        assert [len(r) for r in rows] == N_BLOCKS
        for r in rows:
            assert (r % 64 == 0).all()
        out[mode] = {n: r // 64 for n, r in zip(N_BLOCKS, rows)}
    return out


@pytest.mark.parametrize("n_blocks", N_BLOCKS)
def test_mode_0_is_the_identity(wave_map, n_blocks):
    np.testing.assert_array_equal(wave_map[0][n_blocks], np.arange(n_blocks))


@pytest.mark.parametrize("n_blocks", N_BLOCKS)
def test_mode_1_is_a_permutation_with_one_ascending_range_per_residue_class(wave_map, n_blocks):
    slot = wave_map[1][n_blocks]
    np.testing.assert_array_equal(np.sort(slot), np.arange(n_blocks))  # a permutation of [0, n_blocks)
    nxt = 0
    for x in range(8):  # the classes in residue order, each one contiguous ascending range that starts where the last ended
        mine = slot[x::8]
        assert len(mine) == (n_blocks - x + 7) // 8
        np.testing.assert_array_equal(mine, nxt + np.arange(len(mine)))
        nxt += len(mine)
    assert nxt == n_blocks


# ---- on the device ---------------------------------------------------------------------------------------------------------

DT, NSTEPS = 2.0**-9, 8
GRID = np.arange(NSTEPS + 1) * DT
F_RECORDS = {"MEAN": 0, "COV_TRIL": 1, "DIFFUSION": 2, "LOGLIK": 4, "NSAVED": 9, "RETCODE": 10}
F_SMOOTHED = {"SMOOTH_MEAN": 11, "SMOOTH_COV_TRIL": 12}


def _solve(pkg, monkeypatch, mode, N, *, alg=1, diffusion="dynamic", smooth=False, kernel="ek_filter_fixed_kernel"):
    """Lorenz-63, order 3, 8 fixed steps, every step saved, want_loglik on, in a fresh context, on the lane filter."""
    monkeypatch.setenv("ODEF_FILTER_ROWS_MAX_N", "0")
    monkeypatch.setenv("ODEF_WAVE_MAP", str(mode))
    vf = orc.vector_field("lorenz63")
    ctx = pkg.Context("lorenz63", 3, alg, N, diffusion=diffusion, smooth=smooth, save_everystep=True, want_loglik=True)
    ctx.set_problem_perturbed(vf.u0, vf.p, 0.0, 1e-2)
    ctx.solve_fixed(GRID)
    assert kernel in ctx.kernel_name(0), ctx.kernel_name(0)
    fields = dict(F_RECORDS)
    if smooth:
        ctx.smooth()
        fields.update(F_SMOOTHED)
    out = {name: ctx.get(f).copy() for name, f in fields.items()}
    ctx.close()
    return out


def _assert_same_bits(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        assert a[name].shape == b[name].shape and a[name].dtype == b[name].dtype, (what, name)
        assert np.array_equal(a[name], b[name], equal_nan=True), f"{what}: {name} differs between the two wave maps"


@pytest.mark.gpu
@pytest.mark.parametrize("lag", ["0", "1000000000"], ids=["in-step", "lagged"])
@pytest.mark.parametrize("N", [453, 512, 577, 1088])  # 7 waves + 5 lanes; 8 waves; 9 waves + 1 lane; 17 waves
def test_xcd_contiguous_map_gives_the_identity_maps_bits(pkg, monkeypatch, N, lag):
    monkeypatch.setenv("ODEF_FILTER_LAG_MAX_N", lag)
    a = _solve(pkg, monkeypatch, 0, N)
    b = _solve(pkg, monkeypatch, 1, N)
    assert (a["RETCODE"] == 0).all() and (a["NSAVED"] == NSTEPS + 1).all() and np.isfinite(a["MEAN"]).all()
    assert np.abs(a["COV_TRIL"][-1]).max(axis=0).min() > 0  # every trajectory's last record was written
    _assert_same_bits(a, b, f"N = {N}")


@pytest.mark.gpu
def test_smoothed_records_after_a_solve_under_either_map(pkg, monkeypatch):
    a = _solve(pkg, monkeypatch, 0, 577, smooth=True)
    b = _solve(pkg, monkeypatch, 1, 577, smooth=True)
    assert np.isfinite(a["SMOOTH_MEAN"]).all() and np.abs(a["SMOOTH_COV_TRIL"][1]).max() > 0
    _assert_same_bits(a, b, "N = 577, smoothed")


@pytest.mark.gpu
def test_mv_diffusion_ek0_under_either_map(pkg, monkeypatch):
    kw = dict(alg=0, diffusion="dynamicMV", kernel="ek_filter_fixed_mv_kernel")
    a = _solve(pkg, monkeypatch, 0, 577, **kw)
    b = _solve(pkg, monkeypatch, 1, 577, **kw)
    assert a["DIFFUSION"].size == (NSTEPS + 1) * 3 * 577 and (a["RETCODE"] == 0).all()
    _assert_same_bits(a, b, "N = 577, dynamicMV EK0")


@pytest.mark.gpu
def test_ieks_under_either_map(pkg, monkeypatch):
    monkeypatch.setenv("ODEF_FILTER_ROWS_MAX_N", "0")
    vf = orc.vector_field("lorenz63")
    ens = pkg.EnsembleProblem(pkg.ODEProblem("lorenz63", vf.u0, (0.0, NSTEPS * DT), vf.p), perturb_scale=1e-2)
    out = {}
    for mode in (0, 1):
        monkeypatch.setenv("ODEF_WAVE_MAP", str(mode))
        sol = pkg.solve_ieks(ens, pkg.IEKS(order=3), pkg.EnsembleHIP(), trajectories=577, dt=DT, adaptive=False, iterations=2)
        assert "ek_filter_fixed_ieks_kernel" in sol.ctx.kernel_name(0), sol.ctx.kernel_name(0)
        assert sol.retcode == ["Success"] * 577
        out[mode] = {name: sol.ctx.get(f).copy() for name, f in {**F_RECORDS, **F_SMOOTHED}.items()}
        sol.ctx.close()
    _assert_same_bits(out[0], out[1], "N = 577, IEKS")


@pytest.mark.gpu
def test_xcd_contiguous_map_against_the_oracle(pkg, monkeypatch):
    """As test_ensemble_parity_with_oracle (tests/test_gpu_parity.py), with its helpers and bars: first and last lanes of waves
    that the map moves, and the single lane of the partial wave."""
    monkeypatch.setenv("ODEF_FILTER_ROWS_MAX_N", "0")
    monkeypatch.setenv("ODEF_WAVE_MAP", "1")
    vf = orc.vector_field("lorenz63")
    N, t1 = 577, NSTEPS * DT
    ens = pkg.EnsembleProblem(pkg.ODEProblem("lorenz63", vf.u0, (0.0, t1), vf.p), perturb_scale=1e-2)
    sol = pkg.solve(ens, pkg.EK1(order=3, smooth=True), pkg.EnsembleHIP(), trajectories=N, dt=DT, adaptive=False)
    assert "ek_filter_fixed_kernel" in sol.ctx.kernel_name(0)
    u0s = orc.ensemble_u0(vf.u0, N, 1e-2)
    np.testing.assert_array_equal(sol.ctx.get(13).T, u0s)
    assert sol.retcode == ["Success"] * N
    alg_o = orc.Alg("EK1", 3, "dynamic", True)
    mf, cf, ms, cs = sol.x_filt_mean(), sol.x_filt_cov(), sol.x_smooth_mean(), sol.x_smooth_cov()
    for i in (0, 63, 64, 127, 128, 300, 511, 512, 575, 576):
        for smoothed, (m, c) in ((False, (mf, cf)), (True, (ms, cs))):
            base, nm, nc = P.oracle_noise(vf, alg_o, u0s[i], dict(tspan=(0.0, t1), dt=DT), smoothed)
            P.check_against_oracle(m[i], c[i], base.means(smoothed=smoothed), base.covs(smoothed=smoothed), vf.d, nm, nc,
                                   f"lorenz63 EK1(3) wave map 1 traj {i} smoothed={smoothed}")
    sol.ctx.close()
