#!/usr/bin/env python3
"""Time the route pass (routes.hip) alone, device resident, on the benchmark graphs.

  c4  complete, n = 32,768, every row, after srt_dense_build_device
      (srt_routes_dense_device: the essential-arc compaction + the route kernel)
  c3  random geometric, n = 20,000, every row (srt_routes_rows_device)
  c5  Barabasi-Albert m = 3, n = 100,000, 4,096 sources (srt_routes_rows_device)

The distance rows are built once and stay on the device; the pass is timed by the HIP events of
srt_route_stats.ms_routes: three warm-up passes, then the median of --reps (>= 5). One JSON line
per configuration goes to --out-dir. The model beside each time: arc visits x 4 B
of distance gathers against the ds_read_b32 rate (128 B/clk/CU x 256 CUs x 2.4 GHz; staging forms
1 and 2) or the L2 gather rate (form 3), plus 12 B written per pair against the measured HBM copy
rate. Needs a GPU; there is no fallback.

usage: python tools/routes_time.py [--configs c4,c3,c5] [--reps 5] [--out-dir profiles/routes]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (first: torch and the library share one HIP runtime)

from shadow_amd import _lib, graphs  # noqa: E402
from shadow_amd.topology import SparseGraph  # noqa: E402

LDS_B32_TBS = 128 * 256 * 2.4e9 / 1e12  # ds_read_b32: 128 B/clk/CU, 256 CUs, 2.4 GHz
L2_GATHER_TBS = 17.0                    # rows shared by every workgroup, gathered from the XCD's L2
HBM_TBS = 6.29                          # measured float4 copy

CONFIGS = {
    "c4": dict(kind="dense", n=32768, seed=4, lat_max=1000, self_max=10, loss_max=500),
    "c3": dict(kind="sparse", n=20000, seed=3, gen="rgg", nsrc=None),
    "c5": dict(kind="sparse", n=100000, seed=5, gen="ba", nsrc=4096),
}


def model(arc_visits, pairs, forms):
    gather = LDS_B32_TBS if not forms & 4 else L2_GATHER_TBS
    ms_gather = arc_visits * 4 / (gather * 1e12) * 1e3
    ms_write = pairs * 12 / (HBM_TBS * 1e12) * 1e3
    return dict(model_ms=ms_gather + ms_write, model_gather_ms=ms_gather, model_write_ms=ms_write,
                gather_rate_tbs=gather, bound="hbm writes" if ms_write > ms_gather else "gathers")


def timed(run, reps):
    for _ in range(3):
        run()
    ms = [run() for _ in range(reps)]
    return statistics.median(ms), min(ms), max(ms)


def time_dense(cfg, reps):
    L = _lib.lib()
    n = cfg["n"]
    ld = (n + 127) // 128 * 128
    w = torch.empty((ld, ld), dtype=torch.int32, device="cuda")
    r = torch.empty((ld, ld), dtype=torch.float64, device="cuda")
    _lib.check(L.srt_gen_complete_device(n, ld, 0, ld, cfg["seed"], cfg["lat_max"], cfg["self_max"],
                                         cfg["loss_max"], w.data_ptr(), r.data_ptr(), None),
               "srt_gen_complete_device")
    lat = torch.empty_like(w)
    rel = torch.empty_like(r)
    bs = _lib.BuildStats()
    _lib.check(L.srt_dense_build_device(n, ld, 0, w.data_ptr(), r.data_ptr(), lat.data_ptr(),
                                        rel.data_ptr(), None, 0, ctypes.byref(bs)),
               "srt_dense_build_device")
    del r, rel
    outs = [torch.empty((n, n), dtype=torch.int32, device="cuda") for _ in range(3)]
    st = _lib.RouteStats()

    def run():
        _lib.check(L.srt_routes_dense_device(n, ld, 0, w.data_ptr(), lat.data_ptr(), 0, n,
                                             *[o.data_ptr() for o in outs], n, None,
                                             ctypes.byref(st)), "srt_routes_dense_device")
        return st.ms_routes

    med, lo, hi = timed(run, reps)
    return dict(rows=n, arcs=int(st.ess_arcs), arc_visits=n * int(st.ess_arcs), pairs=n * n,
                ms_tables=bs.ms_total, ms_routes=med, ms_min=lo, ms_max=hi, max_hops=st.max_hops,
                stage_forms=st.stage_forms, includes="essential-arc compaction + route kernel")


def time_sparse(cfg, reps):
    n = cfg["n"]
    g = graphs.random_geometric(n, seed=cfg["seed"]) if cfg["gen"] == "rgg" else \
        graphs.barabasi_albert(n, seed=cfg["seed"])
    sg = SparseGraph(g.n, False, g.src, g.dst, g.lat_ns, g.loss)
    nsrc = cfg["nsrc"] or n
    lat = torch.empty((nsrc, n), dtype=torch.int32, device="cuda")
    rel = torch.empty((nsrc, n), dtype=torch.float64, device="cuda")
    bs = _lib.BuildStats()
    dsrc = None
    if cfg["nsrc"]:
        dsrc = torch.arange(0, n, n // nsrc, dtype=torch.int32, device="cuda")[:nsrc].contiguous()
        sg.rows_list(dsrc.data_ptr(), nsrc, lat.data_ptr(), rel.data_ptr(), stats=bs)
    else:
        sg.rows(0, n, lat.data_ptr(), rel.data_ptr(), stats=bs)
    del rel
    outs = [torch.empty((nsrc, n), dtype=torch.int32, device="cuda") for _ in range(3)]
    st = _lib.RouteStats()

    def run():
        sg.routes_rows(lat.data_ptr(), nsrc, *[o.data_ptr() for o in outs],
                       srcs_ptr=None if dsrc is None else dsrc.data_ptr(), stats=st)
        return st.ms_routes

    med, lo, hi = timed(run, reps)
    out = dict(rows=nsrc, arcs=int(sg.arcs), arc_visits=nsrc * int(sg.arcs), pairs=nsrc * n,
               ms_tables=bs.ms_total, ms_routes=med, ms_min=lo, ms_max=hi, max_hops=st.max_hops,
               stage_forms=st.stage_forms, includes="route kernel")
    sg.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c4,c3,c5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "routes"))
    a = ap.parse_args()
    assert a.reps >= 5, "the median of at least five passes"
    assert torch.cuda.is_available(), "routes_time.py needs a GPU"
    os.makedirs(a.out_dir, exist_ok=True)
    for name in a.configs.split(","):
        cfg = CONFIGS[name]
        res = time_dense(cfg, a.reps) if cfg["kind"] == "dense" else time_sparse(cfg, a.reps)
        res.update(model(res["arc_visits"], res["pairs"], res["stage_forms"]))
        res.update(config=name, n=cfg["n"], reps=a.reps, warmup=3,
                   device=torch.cuda.get_device_name(0),
                   fraction_of_model=res["model_ms"] / res["ms_routes"])
        line = json.dumps(res)
        print(line, flush=True)
        with open(os.path.join(a.out_dir, f"{name}.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
