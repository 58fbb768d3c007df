"""tests/sparse_graphs.py without a GPU: every helper builds its graph and asserts its own
property against the oracle or against srt_canon_build (the helpers assert before they hand a
graph out; the checks here restate what test_gpu_sparse_edges.py rests on)."""
import numpy as np
import pytest

import level_graphs as lg
import sparse_graphs as sg
from level_graphs import MS, U64_MAX


@pytest.mark.parametrize("n_losses", [200, 300])
@pytest.mark.parametrize("target", [1022, 1023, 1024])
def test_two_part_tail_distance_and_blind_probe(native, target, n_losses):
    g = sg.two_part(target, n_losses)
    ecc, h = g.ecc, g.head
    assert int(ecc[h:].max()) == target and int(ecc[:h].max()) < 1002
    assert 2 * int(ecc[0]) <= 1022  # the probe source sees nothing of the tail
    over = int((ecc >= 1023).sum())
    assert (over > 0) == (target >= 1023)
    assert int((ecc >= 1023 - 20).sum()) >= max(over, 1)
    d = lg.oracle_table(g)["lat_int"]
    assert (d[:h, h:] == U64_MAX).all() and (d[h:, h:] != U64_MAX).all()
    assert (sg.distinct_reliabilities(g) <= 256) == (n_losses == 200)


@pytest.mark.parametrize("n_losses", [200, 300])
def test_fan_first_level_fills_the_indexed_blocks(native, n_losses):
    g = sg.fan(n_losses=n_losses)
    deg = sg.canon(g)["deg"][g.first]
    assert len(g.first) == 12 and int(deg.sum()) > 16384 + int(deg.max())
    # some hub's arcs begin past the 256th 64-arc block whatever the hubs' order in the bucket
    assert int(deg.sum()) - int(deg.max()) > 256 * 64


@pytest.mark.parametrize("d,n_losses", [(64, 200), (4094, 200), (4095, 200), (4096, 200),
                                        (32767, 300)])
def test_star_hub_degree(native, d, n_losses):
    g = sg.star(d, n_losses)
    c = sg.canon(g)
    assert g.n == d + 1 and int(c["deg"][0]) == d and int(c["deg"].max()) == d
    assert (sg.distinct_reliabilities(g) <= 256) == (n_losses == 200)


@pytest.mark.parametrize("w", [127, 128, 254, 255, 256])
def test_heavy_pendants_largest_weight(native, w):
    g = sg.heavy_pendants(w)
    c = sg.canon(g)
    assert c["max_w_q"] == w and c["q"] == MS
    assert int((c["w"] == w).sum()) == 2 * 300  # both directions of every pendant's arc
    assert 2 * int(lg.row_eccentricity(g)[0]) <= 1022


@pytest.mark.parametrize("k", [256, 257])
def test_loss_table_distinct_reliabilities(native, k):
    assert sg.distinct_reliabilities(sg.loss_table(k)) == k


@pytest.mark.parametrize("arcs,n", [(40000, 2048), (2 ** 20 - 2, 16384), (2 ** 20, 16384)])
def test_many_arcs_count(native, arcs, n):
    g = sg.many_arcs(arcs, n=n)
    c = sg.canon(g)
    assert c["arcs"] == arcs and int(c["rp"][-1]) == arcs
    assert (int(c["rp"][n - 1]) >= 2 ** 20 - 256) == (arcs >= 2 ** 20 - 2)


@pytest.mark.parametrize("total", [65534, 65535])
def test_bound_path_undirected_distance_bound(native, total):
    g = sg.bound_path(total)
    assert sg.canon(g)["dist_bound"] == total
    d = lg.oracle_table(g)["lat_int"]
    assert int(d[0, g.n - 1]) == total * MS == int(d.max())


@pytest.mark.parametrize("hops,total", [(434, 65534), (435, 65685)])
def test_bound_path_directed_distance_bound(native, hops, total):
    g = sg.bound_path(hops * 151, directed=True)
    assert g.n == hops + 1 and sg.canon(g)["dist_bound"] == total
    assert lg.largest_distance(g) == total
    assert (total < 0xFFFF) == (hops == 434)
