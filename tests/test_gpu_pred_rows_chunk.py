"""lvl_pred_rows_kernel's units of several sub-chunks (levels.hip): a workgroup keeps its 16 targets
and walks up to four 512-source sub-chunks of one 2,048-source chunk back to back, rebuilding
between them what a sub-chunk leaves behind -- the sidx fill, the claimed word, the level bits, the
bounds that the level planes overwrote, the sub-chunk's words and sources.

SRT_FORM pkw=4 forces whole-chunk units at any share, pkw=3 one sub-chunk per unit, pkw=1 takes the
rule (narrow shares keep one sub-chunk), pkw=2 is lvl_pred_kernel's target-major words and the
transpose. Every build is forced through the levels (SRT_FORM levels=1, dist_enc 12); each case
checks the pkw=4 build against the CPU oracle (latency bit-exact, reliability within 1e-12
relative) and bit for bit against the pkw=3 and pkw=2 builds. The shapes are the smallest with a
unit of more than one sub-chunk: 20 words (16 + 4), 33 words (16 + 16 + 1) and 68 words (a
four-sub-chunk unit, then a chunk of one 4-word sub-chunk)."""
import numpy as np
import pytest
from conftest import set_form

import level_graphs as lg
import pred_chunk_graphs as pg
from shadow_amd import _lib
from shadow_amd._lib import ALGO_DENSE_FW
from shadow_amd.topology import build_tables

pytestmark = pytest.mark.gpu
REL_TOL = 1e-12
LEVELS = 12

_have = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    pg.clear()


def _graph(kind):
    if kind == "ties":  # test_gpu_pred_rows_w4.py's
        return pg.complete(640, 11, 3)
    if kind == "deep_middle":
        return pg.deep_middle()
    if kind == "five_sub":
        return pg.complete(2176, 5, 200)
    raise KeyError(kind)


def _require_kernel():
    """A library without lvl_pred_rows_kernel would read every pkw != 0, 2 as its target-major
    form and pass the comparisons below unchanged."""
    if "k" not in _have:
        with open(_lib.LIB_PATH, "rb") as f:
            _have["k"] = b"lvl_pred_rows_kernel" in f.read()
    assert _have["k"], "this library has no lvl_pred_rows_kernel"


def _build(monkeypatch, g, pkw, ngpus=None, **form):
    _require_kernel()
    set_form(monkeypatch, levels="1", pkw=pkw, **form)
    lat, rel, st = build_tables(g.n, g.directed, g.src, g.dst, g.lat_ns, g.loss,
                                algo=ALGO_DENSE_FW, ngpus=ngpus)
    assert st.dist_enc == LEVELS, st.dist_enc
    return lat, rel, st


def _same(what, a, b):
    assert np.array_equal(a[0], b[0]), what
    diff = np.argwhere(a[1].view(np.uint64) != b[1].view(np.uint64))
    assert diff.size == 0, (what, len(diff), diff[:5].tolist())


def _all_forms(monkeypatch, g, what, ngpus=None, also=(), **form):
    """The pkw=4 build against the oracle, and bit for bit against pkw=3, pkw=2 and `also`;
    -> the stats of the pkw=4 and the pkw=2 builds."""
    b4 = _build(monkeypatch, g, "4", ngpus=ngpus, **form)
    lat, rel, st = b4
    exp = lg.oracle_table(g)
    bad = np.argwhere(lat != np.asarray(exp["lat_int"], np.uint64))
    assert bad.size == 0, f"{what}: {len(bad)} latency mismatches, first {bad[:5].tolist()}"
    err = np.abs(rel - exp["rel"]) / np.maximum(np.abs(exp["rel"]), 1e-300)
    assert float(err.max()) <= REL_TOL, f"{what}: max rel error {err.max()}"
    st2 = None
    for pkw in ("3", "2") + tuple(also):
        other = _build(monkeypatch, g, pkw, ngpus=ngpus, **form)
        _same(f"{what}: pkw=4 against pkw={pkw}", b4, other)
        if pkw == "2":
            st2 = other[2]
    return st, st2


@pytest.mark.parametrize("bcap", ["2048", "1", "-1"])
def test_chunk_two_sub_buckets(gpu, monkeypatch, bcap):
    """n = 640, 1-3 ms arcs: 20 words, one unit of two sub-chunks (16 and 4 words). The chunk's
    bucket is filtered per sub-chunk inside one unit: buckets that cannot overflow, buckets that
    all do, no pre-pass; the pre-pass counters are the pkw=2 build's."""
    st, st2 = _all_forms(monkeypatch, _graph("ties"), f"ties bcap={bcap}", bcap=bcap)
    assert (st.pred_near, st.pred_near_over) == (st2.pred_near, st2.pred_near_over)
    if bcap == "2048":
        assert st.pred_near == 2048 and st.pred_near_over == 0, (st.pred_near, st.pred_near_over)
    elif bcap == "1":
        assert st.pred_near == 1 and st.pred_near_over > 0, (st.pred_near, st.pred_near_over)
    else:
        assert st.pred_near == 0, st.pred_near


def test_chunk_deep_middle(gpu, monkeypatch):
    """n = 1,056 (sub-chunks of 16, 16 and 1 words in one unit): only sources 512..1023 have
    pairs at levels 13..20, so a claimed word, level bits or bounds carried from one sub-chunk
    to the next change the middle sub-chunk's words or its neighbours'."""
    st, _ = _all_forms(monkeypatch, _graph("deep_middle"), "deep_middle")
    assert 8 <= st.levels <= 31, st.levels
    assert st.levels == 20, st.levels


@pytest.mark.parametrize("bcap", ["2048", "8"])
def test_chunk_five_sub(gpu, monkeypatch, bcap):
    """n = 2,176 complete, 1-200 ms arcs (68 words: a four-sub-chunk unit, then a chunk of one
    4-word sub-chunk), at least 4 levels, with the pre-pass: buckets that cannot overflow, and
    buckets of 8 entries (some over, some not). pkw=1, whichever form the rule picks, is
    bit-equal to both forced forms."""
    g = _graph("five_sub")
    st, st2 = _all_forms(monkeypatch, g, f"five_sub bcap={bcap}", also=("1",), bcap=bcap)
    assert st.levels >= 4, st.levels
    assert st.pred_near == int(bcap), st.pred_near
    assert (st.pred_near, st.pred_near_over) == (st2.pred_near, st2.pred_near_over)
    if bcap == "8":
        assert 0 < st.pred_near_over < g.n * 2, st.pred_near_over
    else:
        assert st.pred_near_over == 0, st.pred_near_over


def test_chunk_five_sub_virtual_ranks(gpu, monkeypatch):
    """The same graph on two row shards of 1,024 and 1,152 rows: src0 != 0 and shares that are
    not whole chunks (units of 16 + 16 and of 16 + 16 + 4 words)."""
    monkeypatch.setenv("SRT_VIRTUAL_RANKS", "2")
    st, _ = _all_forms(monkeypatch, _graph("five_sub"), "five_sub x2", ngpus=1, bcap="2048")
    assert st.levels >= 4, st.levels
