"""CPU: mf_plan.h (gpmf_mes_argbest's tiling) pinned at its edges by the host compiler; suggest_multifidelity's argument errors."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from bayesianoptimization_amd import suggest_multifidelity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = r"""
#include "mf_plan.h"
#include <cstdio>
#include <initializer_list>
using namespace gpbo;
int main() {
  for (long NP : {64L, 192L, 256L, 320L, 576L, 16384L}) {
    printf("%ld %d", NP, mf_chunks(NP));
    for (int r : {0, mf_chunks(NP) - 1}) printf(" %d", mf_chunk_stages(NP, r));
    printf("\n");
  }
  printf("tiles %d %d %d %d\n", mf_tile_a(1, 0), mf_tile_b(1, 0), mf_tile_a(0, 7), mf_tile_b(0, 7));
  printf("last %d %d %d\n", mf_tile_last_stage(3, 20), mf_tile_last_stage(19, 20), mf_tile_last_stage(31, 20));
  printf("blocks %ld %ld %ld\n", (long)mf_blocks(1), (long)mf_blocks(32), (long)mf_blocks(33));
  for (int DP : {4, 8, 16, 32, 64}) printf("lds %d %ld\n", DP, (long)mf_lds_bytes(DP));
  return 0;
}
"""


def test_mf_plan_edges(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "p.cpp", tmp_path / "p"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-I", os.path.join(ROOT, "bayesianoptimization_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    # NP, chunks, stages of the first and of the last chunk: the triangular stop, ragged last chunks
    assert out[:6] == ["64 1 4 4", "192 1 12 12", "256 1 16 16", "320 2 16 20", "576 3 16 36", "16384 64 16 1024"]
    assert out[6] == "tiles 16 31 7 8" and out[7] == "last 3 19 19" and out[8] == "blocks 1 1 2"
    lds = dict(tuple(map(int, ln.split()[1:])) for ln in out[9:14])
    assert lds[4] == lds[8] == lds[16] == 28416 and lds[32] == 33792 and lds[64] == 50176 and max(lds.values()) <= 65536


BAD = [(dict(fidelity="nope"), "fidelity must be one"), (dict(target=2.0), "target"), (dict(cost=(0.0, 1.0)), "cost"),
       (dict(cost=(1.0, -1.0)), "cost"), (dict(cost=(np.inf, 0.0)), "cost"), (dict(n_samples=65), "n_samples"), (dict(n_samples=1.5), "n_samples"),
       (dict(n_random=0), "n_random"), (dict(n_star=0), "n_star"), (dict(n_features=0), "n_features"), (dict(floor_sigmas=-1.0), "floor_sigmas"),
       (dict(fidelities=[0.5, 3.0]), "fidelities"), (dict(fidelities=[]), "fidelities")]


@pytest.mark.parametrize("kw,match", BAD)
def test_suggest_multifidelity_argument_errors(kw, match):
    space = types.SimpleNamespace(keys=["a", "s"], bounds=np.array([[0.0, 1.0], [0.1, 1.0]]))
    fake = types.SimpleNamespace(_space=space, _gp=None, _random_state=None)      # no engine: every error comes before the gate
    with pytest.raises(ValueError, match=match):
        suggest_multifidelity(fake, **{"fidelity": "s", **kw})
    with pytest.raises(NotImplementedError, match="not on the engine"):
        suggest_multifidelity(fake, "s")
