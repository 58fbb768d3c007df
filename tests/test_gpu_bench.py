"""bench.py keeps the driver's JSON-line contract (one line on rank 0, the BASELINE metric, the
roofline and, under --full, the CPU-baseline objects) and its full-size parity spot check holds --
run on the small C2 workload so it finishes in seconds. A plain run (no --full) only times its
steps and can write the last step's tables (--dump-outputs)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["c2", "c3"])
def test_bench_json_line_contract(workload):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", workload,
                          "--steps", "2", "--warmup", "1", "--cpu-seconds", "1", "--full"],
                         capture_output=True, text=True, timeout=110, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [x for x in out.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["metric"].startswith("routing-table build time") and d["unit"] == "node-pairs/s"
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0
    rf = d["roofline"]
    assert rf["bound"] in ("hbm", "mfma") and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    cb = d["cpu_baseline"]
    assert cb["kind"] in ("port", "reference") and cb["cores"] == 1 and cb["value"] > 0
    assert cb["all_cores"]["cores"] >= 1 and cb["all_cores"]["value"] > 0
    assert d["parity"]["lat_bit_exact"] is True
    assert d["parity"]["rel_max_rel_err"] <= 1e-12
    assert d["parity"]["rows_checked"] >= 4 and d["parity"]["tied_pairs"] >= 0
    assert 0.0 <= d["parity"]["tied_frac"] < 0.5


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """Without --full the run times its steps and prints the line: no tie-count build, no oracle
    leg. --dump-outputs writes the last timed step's tables (C2 fits whole) as float64."""
    import numpy as np
    d = tmp_path / "out"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c2",
                          "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)],
                         capture_output=True, text=True, timeout=110, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [x for x in out.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, out.stdout
    r = json.loads(lines[0])
    assert r["metric"].startswith("routing-table build time") and r["unit"] == "node-pairs/s"
    assert r["higher_is_better"] is True and r["dtype"] in ("u16", "u32")
    assert r["steps"] == 3 and out.stderr.count("[bench] step ") == 3
    assert r["ms_per_step"] > 0
    # value = n^2 / (seconds per step); ms_per_step is rounded to 1e-3 ms
    assert abs(1000.0 * 1000.0 / r["value"] * 1e3 - r["ms_per_step"]) <= 1e-3
    assert r["cpu_baseline"] is None and r["parity"] is None
    lat, rel, rows = (np.load(d / f"{k}.npy") for k in ("lat", "rel", "rows"))
    assert sorted(os.listdir(d)) == ["lat.npy", "rel.npy", "rows.npy"]
    assert lat.dtype == rel.dtype == rows.dtype == np.float64
    assert lat.shape == rel.shape == (1000, 1000) and np.array_equal(rows, np.arange(1000.0))
    off = ~np.eye(1000, dtype=bool)
    assert (lat[off] >= 1).all() and (lat[off] <= 300).all()  # quanta: at most the direct arc
    assert (rel[off] > 0).all() and (rel[off] <= 1).all()
