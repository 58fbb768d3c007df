#!/usr/bin/env python3
"""Time the envelope pass (envelope.hip) alone, device resident, on the benchmark graphs, beside
the route pass of the same run.

  c4  complete, n = 32,768, every row, after srt_dense_build_device
      (srt_envelope_dense_device: the essential-arc compaction, the reliability gather and the
      envelope kernel; srt_routes_dense_device: the compaction and the route kernel)
  c3  random geometric, n = 20,000, every row (srt_envelope_rows_device, srt_routes_rows_device)
  c5  Barabasi-Albert m = 3, n = 100,000, 4,096 sources (the same two)

The distance rows are built once and stay on the device; each pass is timed by the HIP events of
its stats (ms_envelope, ms_routes): three warm-up passes, then the median of --reps (>= 5). One
JSON line per configuration goes to --out-dir: the two times and their ratio, the sweeps, and the
tied, exposed and sensitive pairs as counts and as fractions of the rows' off-diagonal pairs.
Needs a GPU; there is no fallback.

usage: python tools/envelope_time.py [--configs c4,c3,c5] [--reps 5] [--out-dir profiles/envelope]
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

CONFIGS = {
    "c4": dict(kind="dense", n=32768, seed=4, lat_max=1000, self_max=10, loss_max=500),
    "c3": dict(kind="sparse", n=20000, seed=3, gen="rgg", nsrc=None),
    "c5": dict(kind="sparse", n=100000, seed=5, gen="ba", nsrc=4096),
}


def timed(run, reps):
    for _ in range(3):
        run()
    ms = [run() for _ in range(reps)]
    return statistics.median(ms), min(ms), max(ms)


def result(rows, n, arcs, bs, es, rs, env, routes):
    pairs = rows * (n - 1)
    return dict(rows=rows, arcs=arcs, pairs=pairs, ms_tables=bs.ms_total,
                ms_envelope=env[0], ms_envelope_min=env[1], ms_envelope_max=env[2],
                ms_routes=routes[0], ms_routes_min=routes[1], ms_routes_max=routes[2],
                envelope_over_routes=env[0] / routes[0], max_sweeps=es.max_sweeps,
                max_hops=rs.max_hops, stage_forms=es.stage_forms,
                tied_pairs=es.tied_pairs, exposed_pairs=es.exposed_pairs,
                sensitive_pairs=es.sensitive_pairs, tied_fraction=es.tied_pairs / pairs,
                exposed_fraction=es.exposed_pairs / pairs,
                sensitive_fraction=es.sensitive_pairs / pairs)


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
    del rel
    outs = [torch.empty((n, n), dtype=torch.int32, device="cuda") for _ in range(3)]
    rs = _lib.RouteStats()

    def run_routes():
        _lib.check(L.srt_routes_dense_device(n, ld, 0, w.data_ptr(), lat.data_ptr(), 0, n,
                                             *[o.data_ptr() for o in outs], n, None,
                                             ctypes.byref(rs)), "srt_routes_dense_device")
        return rs.ms_routes

    routes = timed(run_routes, reps)
    del outs
    lo, hi = (torch.empty((n, n), dtype=torch.float64, device="cuda") for _ in range(2))
    es = _lib.EnvelopeStats()

    def run_envelope():
        _lib.check(L.srt_envelope_dense_device(n, ld, 0, w.data_ptr(), r.data_ptr(), lat.data_ptr(),
                                               0, n, lo.data_ptr(), hi.data_ptr(), n, None,
                                               ctypes.byref(es)), "srt_envelope_dense_device")
        return es.ms_envelope

    env = timed(run_envelope, reps)
    out = result(n, n, int(rs.ess_arcs), bs, es, rs, env, routes)
    out["includes"] = "essential-arc compaction (both), reliability gather + envelope kernel"
    return out


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
    sp = None if dsrc is None else dsrc.data_ptr()
    outs = [torch.empty((nsrc, n), dtype=torch.int32, device="cuda") for _ in range(3)]
    rs = _lib.RouteStats()

    def run_routes():
        sg.routes_rows(lat.data_ptr(), nsrc, *[o.data_ptr() for o in outs], srcs_ptr=sp, stats=rs)
        return rs.ms_routes

    routes = timed(run_routes, reps)
    del outs
    lo, hi = (torch.empty((nsrc, n), dtype=torch.float64, device="cuda") for _ in range(2))
    es = _lib.EnvelopeStats()

    def run_envelope():
        sg.envelope_rows(lat.data_ptr(), nsrc, lo.data_ptr(), hi.data_ptr(), srcs_ptr=sp, stats=es)
        return es.ms_envelope

    env = timed(run_envelope, reps)
    out = result(nsrc, n, int(sg.arcs), bs, es, rs, env, routes)
    out["includes"] = "envelope kernel; route kernel"
    sg.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c4,c3,c5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "envelope"))
    a = ap.parse_args()
    assert a.reps >= 5, "the median of at least five passes"
    assert torch.cuda.is_available(), "envelope_time.py needs a GPU"
    os.makedirs(a.out_dir, exist_ok=True)
    for name in a.configs.split(","):
        cfg = CONFIGS[name]
        res = time_dense(cfg, a.reps) if cfg["kind"] == "dense" else time_sparse(cfg, a.reps)
        res.update(config=name, n=cfg["n"], reps=a.reps, warmup=3,
                   device=torch.cuda.get_device_name(0))
        line = json.dumps(res)
        print(line, flush=True)
        with open(os.path.join(a.out_dir, f"{name}.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
