#!/usr/bin/env python3
"""Time the split-load pass (splitload.hip) alone, device resident, on the benchmark graphs.

  c4  complete, n = 32,768, every row, after srt_dense_build_device (srt_split_load_dense_device:
      the timed span is the split-load pass; the essential-arc compaction is outside the events)
  c3  random geometric, n = 20,000, every row (srt_split_load_rows_device)
  c5  Barabasi-Albert m = 3, n = 100,000, 4,096 sources (srt_split_load_rows_device)

Uniform demand (1 for every pair). The distance rows are built once and stay on the device; each
pass runs the route pass (ms_routes), the canonical load pass over the rows it wrote (ms_load) and
the split-load pass over the distance rows (ms_split; HIP events around the pass alone: its
stream-ordered scratch allocation, a 16-byte memset, the kernel and the 16-byte copy of its
counts): three warm-up passes, then the median of --reps (>= 5). A second series gives every row
one unit of demand, at one target: staging, the three walks of the in-lists, the counters and the
sweeps run as before, while almost every share is zero, so the f64 adds into load, inflow and
through shrink to the paths of one pair per row. ms_uniform_minus_one_target is the difference of
the two series: an inference about what the f64 adds cost, not a measurement of them (the
one-target run also branches differently, and the two contend differently). One JSON line per
configuration goes to --out-dir. Needs a GPU; there is no fallback.

usage: python tools/split_load_time.py [--configs c4,c3,c5] [--reps 5] [--out-dir profiles/split_load]
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

SPAN = "split-load pass: scratch allocation, kernel, counts copy"
CONFIGS = {
    "c4": dict(kind="dense", n=32768, seed=4, lat_max=1000, self_max=10, loss_max=500),
    "c3": dict(kind="sparse", n=20000, seed=3, gen="rgg", nsrc=None),
    "c5": dict(kind="sparse", n=100000, seed=5, gen="ba", nsrc=4096),
}


def timed(run, reps):
    """run() -> (ms_routes, ms_load, ms_split); medians over reps after three warm-up passes, and
    the extremes of ms_split."""
    for _ in range(3):
        run()
    got = [run() for _ in range(reps)]
    split = [g[2] for g in got]
    return (statistics.median(g[0] for g in got), statistics.median(g[1] for g in got),
            statistics.median(split), min(split), max(split))


def one_target_demand(dem, srcs):
    """One unit of demand per row, half the vertex range away from the row's source."""
    rows, n = dem.shape
    dem.zero_()
    r = torch.arange(rows, device=dem.device)
    dem[r, (srcs.to(torch.int64) + n // 2) % n] = 1


def summarize(load, through, totals, st):
    tot = totals.cpu().numpy().astype("uint64")
    return dict(loaded_arcs=int((load > 0).sum().item()), load_sum=float(load.sum().item()),
                load_max=float(load.max().item()), through_max=float(through.max().item()),
                routed=int(tot[0]), unrouted=int(tot[1]), self_demand=int(tot[2]),
                tied_pairs=int(st.tied_pairs), max_sweeps=st.max_sweeps, forms=st.forms)


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
    pred = torch.empty((n, n), dtype=torch.int32, device="cuda")
    hops = torch.empty((n, n), dtype=torch.int32, device="cuda")
    rs = _lib.RouteStats()
    _lib.check(L.srt_routes_dense_device(n, ld, 0, w.data_ptr(), lat.data_ptr(), 0, n,
                                         pred.data_ptr(), None, hops.data_ptr(), n, None,
                                         ctypes.byref(rs)), "srt_routes_dense_device")
    cap = int(rs.ess_arcs)
    rowptr = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    tails = torch.empty(cap, dtype=torch.int32, device="cuda")
    iload = torch.empty(cap, dtype=torch.int64, device="cuda")
    ithrough = torch.empty(n, dtype=torch.int64, device="cuda")
    load = torch.empty(cap, dtype=torch.float64, device="cuda")
    through = torch.empty(n, dtype=torch.float64, device="cuda")
    totals = torch.empty(3, dtype=torch.int64, device="cuda")
    dem = torch.empty((n, n), dtype=torch.int64, device="cuda")
    narcs = ctypes.c_int64()
    ls = _lib.LinkLoadStats()
    st = _lib.SplitLoadStats()

    def run():
        _lib.check(L.srt_routes_dense_device(n, ld, 0, w.data_ptr(), lat.data_ptr(), 0, n,
                                             pred.data_ptr(), None, hops.data_ptr(), n, None,
                                             ctypes.byref(rs)), "srt_routes_dense_device")
        _lib.check(L.srt_link_load_dense_device(n, ld, 0, w.data_ptr(), lat.data_ptr(), 0, n,
                                                pred.data_ptr(), hops.data_ptr(), n, dem.data_ptr(),
                                                n, cap, rowptr.data_ptr(), tails.data_ptr(),
                                                iload.data_ptr(), ctypes.byref(narcs),
                                                ithrough.data_ptr(), totals.data_ptr(), None,
                                                ctypes.byref(ls)), "srt_link_load_dense_device")
        _lib.check(L.srt_split_load_dense_device(n, ld, 0, w.data_ptr(), lat.data_ptr(), 0, n,
                                                 dem.data_ptr(), n, cap, rowptr.data_ptr(),
                                                 tails.data_ptr(), load.data_ptr(),
                                                 ctypes.byref(narcs), through.data_ptr(),
                                                 totals.data_ptr(), None, ctypes.byref(st)),
                   "srt_split_load_dense_device")
        return rs.ms_routes, ls.ms_load, st.ms_split

    one_target_demand(dem, torch.arange(n, device="cuda"))
    _, _, skel, _, _ = timed(run, reps)
    dem.fill_(1)
    ms_routes, ms_load, med, lo, hi = timed(run, reps)
    out = dict(rows=n, arcs=int(narcs.value), pairs=n * n, ms_tables=bs.ms_total,
               ms_routes=ms_routes, ms_load=ms_load, ms_split=med, ms_min=lo, ms_max=hi,
               ms_split_one_target=skel,
               includes=SPAN + " (ms_routes: essential-arc compaction + route kernel)")
    out.update(summarize(load, through, totals, st))
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
    if cfg["nsrc"]:
        dsrc = torch.arange(0, n, n // nsrc, dtype=torch.int32, device="cuda")[:nsrc].contiguous()
        sg.rows_list(dsrc.data_ptr(), nsrc, lat.data_ptr(), rel.data_ptr(), stats=bs)
        srcs_ptr = dsrc.data_ptr()
    else:
        dsrc = torch.arange(n, dtype=torch.int32, device="cuda")
        sg.rows(0, n, lat.data_ptr(), rel.data_ptr(), stats=bs)
        srcs_ptr = None
    del rel
    pred = torch.empty((nsrc, n), dtype=torch.int32, device="cuda")
    hops = torch.empty((nsrc, n), dtype=torch.int32, device="cuda")
    dem = torch.empty((nsrc, n), dtype=torch.int64, device="cuda")
    arcs = max(int(sg.arcs), 1)
    iload = torch.empty(arcs, dtype=torch.int64, device="cuda")
    ithrough = torch.empty(n, dtype=torch.int64, device="cuda")
    load = torch.empty(arcs, dtype=torch.float64, device="cuda")
    through = torch.empty(n, dtype=torch.float64, device="cuda")
    totals = torch.empty(3, dtype=torch.int64, device="cuda")
    rs = _lib.RouteStats()
    ls = _lib.LinkLoadStats()
    st = _lib.SplitLoadStats()

    def run():
        sg.routes_rows(lat.data_ptr(), nsrc, pred.data_ptr(), None, hops.data_ptr(),
                       srcs_ptr=srcs_ptr, stats=rs)
        for t in (iload, ithrough, load, through, totals):
            t.zero_()
        torch.cuda.synchronize()
        sg.link_load_rows(nsrc, pred.data_ptr(), hops.data_ptr(), dem.data_ptr(), iload.data_ptr(),
                          ithrough.data_ptr(), totals.data_ptr(), srcs_ptr=srcs_ptr, stats=ls)
        totals.zero_()
        torch.cuda.synchronize()
        sg.split_load_rows(lat.data_ptr(), nsrc, dem.data_ptr(), load.data_ptr(),
                           through.data_ptr(), totals.data_ptr(), srcs_ptr=srcs_ptr, stats=st)
        return rs.ms_routes, ls.ms_load, st.ms_split

    one_target_demand(dem, dsrc)
    _, _, skel, _, _ = timed(run, reps)
    dem.fill_(1)
    ms_routes, ms_load, med, lo, hi = timed(run, reps)
    out = dict(rows=nsrc, arcs=int(sg.arcs), pairs=nsrc * n, ms_tables=bs.ms_total,
               ms_routes=ms_routes, ms_load=ms_load, ms_split=med, ms_min=lo, ms_max=hi,
               ms_split_one_target=skel, includes=SPAN + " (ms_routes: route kernel)")
    out.update(summarize(load, through, totals, st))
    sg.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c4,c3,c5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "split_load"))
    a = ap.parse_args()
    assert a.reps >= 5, "the median of at least five passes"
    assert torch.cuda.is_available(), "split_load_time.py needs a GPU"
    os.makedirs(a.out_dir, exist_ok=True)
    for name in a.configs.split(","):
        cfg = CONFIGS[name]
        res = time_dense(cfg, a.reps) if cfg["kind"] == "dense" else time_sparse(cfg, a.reps)
        res.update(config=name, n=cfg["n"], reps=a.reps, warmup=3,
                   device=torch.cuda.get_device_name(0),
                   split_over_load=res["ms_split"] / res["ms_load"],
                   split_over_routes=res["ms_split"] / res["ms_routes"],
                   ns_per_pair=res["ms_split"] * 1e6 / res["pairs"],
                   ms_uniform_minus_one_target=res["ms_split"] - res["ms_split_one_target"])
        line = json.dumps(res)
        print(line, flush=True)
        with open(os.path.join(a.out_dir, f"{name}.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
