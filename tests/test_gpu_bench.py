"""GPU (-m gpu): what a plain `bench.py` run measures and what it leaves to `--full`.

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints its line; the measured peak, PMC traffic,
parity with the reference, CPU baseline, the other configs and ms/suggest come only with --full, and do not change what the
timed steps compute.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("cpu_baseline", "configs", "suggest_ms", "suggest_ms_fixed_total", "parity")


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("config,M,dtype", [("C2", 65536, "f64"), ("C5", 1 << 18, "f32")])
def test_plain_run_prints_the_headline_and_nothing_that_takes_work_of_its_own(tmp_path, config, M, dtype):
    d = _bench("--config", config, "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert d["unit"] == "candidates/s" and d["higher_is_better"] is True and d["dtype"] == dtype
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(M / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert not set(FULL_ONLY) & set(d)
    assert not {"peak_measured", "traffic_note"} & set(d["roofline"]) and d["roofline"]["frac"] > 0
    assert list(d)[-1] == "summary"
    if config == "C5":      # two GPs whose fits overlap: no fit was timed alone
        assert d["step_breakdown_ms"]["fit"] is None and d["step_breakdown_ms"]["fits_overlapped_wall"] > 0
        assert set(d["roofline_fit"]) == {"note"}
    assert np.load(tmp_path / "acq_values.npy").size == M
    assert int(np.load(tmp_path / "best_index.npy")[0]) == d["best"]["index"]


def test_full_run_adds_the_measured_peak_and_the_parity_and_computes_the_same_step(tmp_path):
    plain = _bench("--config", "C2", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "plain"))
    full = _bench("--config", "C2", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "full"),
                  "--full", "--no-cpu-baseline", "--no-suggest")
    assert full["parity"]["argmin_equals_reference"] and full["parity"]["top10_equals_reference"]
    assert full["roofline"]["peak_measured"] > 0 and "traffic_note" in full["roofline"]
    assert "cpu_baseline" not in full and "suggest_ms" not in full
    assert list(full)[-1] == "summary"
    for name in ("best_index", "best_value", "topk_index", "topk_value", "acq_values"):
        assert np.array_equal(np.load(tmp_path / "plain" / f"{name}.npy"), np.load(tmp_path / "full" / f"{name}.npy")), name
    assert plain["best"] == full["best"]
