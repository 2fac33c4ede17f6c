"""GPU (-m gpu): the int8 posterior GEMM (posterior_i8.hip) where its tiling is uneven, at the largest model it serves, and
across the slab widths of its walk (posterior_plan.h, i8_slab_width):

  * ragged last row chunk and uneven waves: N = 2100 (NP = 2112: the last 128-row chunk has two waves without rows), N = 2048,
    N = 2049 (NP = 2112 again, from its lower edge): sigma of the default path within 1e-12 of s_y of the fp64 GEMM
    (GPBO_POST_KERNEL=3, debug build), mu bitwise equal, the bar of test_gpu_int8_posterior.py's C3 case;
  * the upper edge NP = 16384 with 3000 candidates (one full slab of 2048 and a partial one) against the fp64 GEMM at the same
    bar.  The device's free memory is asked before anything runs, and the case is skipped only if it is below what the model
    needs; any error after that fails the test;
  * width independence: the same candidates with GPBO_KSTAR_GB forcing the smallest slab (128 candidates), with a budget below
    the rule's width, with the default (six full slabs and a partial one) and as a 128-candidate batch across a slab edge (kept
    on the slab route with the debug build's GPBO_SMALL_MAX=0) give bitwise equal mu and sd."""
import ctypes
import os

import numpy as np
import pytest

from bayesianoptimization_amd import workloads as W
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu


def _posterior(engine, path, ym, ys, kstar_gb=None, small_max=None):
    env = {"GPBO_POST_KERNEL": path, "GPBO_KSTAR_GB": kstar_gb, "GPBO_SMALL_MAX": small_max}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        return engine.posterior(0, ym, ys)
    finally:
        for k in env:
            os.environ.pop(k, None)


def _problem(N, d, seed):
    rng = np.random.RandomState(seed)
    X = rng.uniform(size=(N, d))
    y = np.sin(3.0 * X.sum(1)) + 0.1 * rng.standard_normal(N)
    return X, y


def _against_fp64(debug_engine, N, M, d=8, seed=5):
    X, y = _problem(N, d, seed)
    Xc = np.random.RandomState(seed + 1).uniform(size=(M, d))
    yn, ym, ys = O.normalize_targets(y)
    debug_engine.fit(X, yn, O.MATERN25, 0.7, 1e-4)
    debug_engine.set_candidates(Xc)
    mu8, sd8 = _posterior(debug_engine, None, ym, ys)
    mu3, sd3 = _posterior(debug_engine, "3", ym, ys)
    d_sd = float(np.max(np.abs(sd8 - sd3)) / ys)
    print(f"N = {N}, M = {M}: max |sd_i8 - sd_f64| / s_y = {d_sd:.3e}, mu bitwise equal: {np.array_equal(mu8, mu3)}")
    assert np.array_equal(mu8, mu3), "mu does not go through the GEMM: bitwise the fp64 path's"
    assert d_sd <= 1e-12, d_sd


@pytest.mark.parametrize("N", [2100, 2048, 2049])
def test_ragged_chunk_and_uneven_waves_match_the_fp64_gemm(debug_engine, N):
    _against_fp64(debug_engine, N, 5000)


def test_widths_of_the_slab_walk_do_not_change_a_bit(debug_engine):
    engine = debug_engine
    # NP = 2048: 14 336 B of digits per candidate, slabs of 16 384 candidates (i8_slab_width).
    # M = 100 000 (Mp = 100 096): six full slabs and one of 1792.
    N, M, d = 2048, 100000, 8
    X, y = _problem(N, d, 11)
    Xc = np.random.RandomState(12).uniform(size=(M, d))
    yn, ym, ys = O.normalize_targets(y)
    engine.fit(X, yn, O.MATERN25, 0.7, 1e-4)
    engine.set_candidates(Xc)
    mu, sd = _posterior(engine, None, ym, ys)
    mu_s, sd_s = _posterior(engine, None, ym, ys, kstar_gb="1e-9")     # one 128-candidate slab at a time
    assert np.array_equal(mu_s, mu) and np.array_equal(sd_s, sd)
    mu_m, sd_m = _posterior(engine, None, ym, ys, kstar_gb="0.1")      # 6912 candidates granted: below the rule's width
    assert np.array_equal(mu_m, mu) and np.array_equal(sd_m, sd)
    at = 3 * 16384 - 64                                                # across a slab edge of the default walk
    engine.set_candidates(Xc[at:at + 128])
    mu_b, sd_b = _posterior(engine, None, ym, ys, small_max="0")       # (debug build: a batch this small is the GEMV path's)
    assert np.array_equal(mu_b, mu[at:at + 128]) and np.array_equal(sd_b, sd[at:at + 128])


def _free_device_bytes():
    """hipMemGetInfo of the HIP runtime this process already runs on (the one libgpbo is linked against)."""
    path = "libamdhip64.so"
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                path = line.split()[-1]
                break
    hip = ctypes.CDLL(path)
    free_b, total_b = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = hip.hipMemGetInfo(ctypes.byref(free_b), ctypes.byref(total_b))
    assert rc == 0, f"hipMemGetInfo: {rc}"
    return free_b.value


def test_upper_edge_np_16384_matches_the_fp64_gemm(debug_engine):
    # K, W = L^-1, W's packed fp64 copy: 2.1 GB each; W's digit planes 0.9 GB; workspaces of the fit: 16 GB asked for
    need = 16e9
    free_b = _free_device_bytes()
    if free_b < need:
        pytest.skip(f"an NP = 16384 model needs about {need / 1e9:.0f} GB of device memory; {free_b / 1e9:.1f} GB are free")
    _against_fp64(debug_engine, 16384, 3000, d=8, seed=21)
