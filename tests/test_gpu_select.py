"""Sparse result fetch on the device: kpe_select_cells (ordered compaction of the verdict
matrix) and kpe_fetch_row_summaries (CalculateSummary per resource) against the same reductions
done on the host over the matrix kpe_fetch returns. The matrix itself is pinned to the oracle by
the parity suites; these tests pin the reductions to the matrix, with exact equality.

Shapes: the smallest at which each mechanism can go wrong. A lane holds 16 cells, a block tile
4096; the selection kernels' persistent grid is 2048 blocks; the summary kernel counts groups of
min(1024, 4096 / R) rows on at most 1536 blocks, with a two-row path for R >= 16."""
import copy
import functools

import numpy as np
import pytest

import kyverno_amd as K
from kyverno_amd._lib import load
from tests.policies import c3_policy_set, c5_policy_set, parity_policy_set, restricted_latest, selector_policy

pytestmark = pytest.mark.gpu

PASS, FAIL, ERROR, SKIP = 1, 2, 4, 5
UNSCORED = {"policies.kyverno.io/scored": "false"}


@pytest.fixture(scope="module")
def engine():
    return K.Engine(ordinal=0)


def _unscored(pols, which):
    pols = copy.deepcopy(pols)
    for i in which:
        pols[i]["metadata"].setdefault("annotations", {}).update(UNSCORED)
    return pols


@functools.lru_cache(maxsize=None)
def program(cfg):
    """(PolicySet, synth seed, synth mix) of a shape's program; some policies are unscored so that
    the FAIL -> warn table is exercised on the device."""
    if cfg == "r1":  # selectors disable autogen: one rule
        pols = _unscored([selector_policy("wild-both", selector={"matchLabels": {"*": "*"}})], [])
        return K.PolicySet(pols), 0xC4, K.SYNTH_SELECTORS
    if cfg == "r3":
        return K.PolicySet([restricted_latest()]), 0xC2, K.SYNTH_MIXED
    if cfg == "r3u":
        return K.PolicySet(_unscored([restricted_latest()], [0])), 0xC2, K.SYNTH_MIXED
    if cfg == "r18":
        pols = _unscored([restricted_latest()] + parity_policy_set()[1:6], [1, 4])
        return K.PolicySet(pols), 21, K.SYNTH_MIXED
    if cfg == "r204":
        pols = c3_policy_set()
        return K.PolicySet(_unscored(pols, range(0, len(pols), 7))), 0xC3, K.SYNTH_C3
    raise KeyError(cfg)


RULES = {"r1": 1, "r3": 3, "r3u": 3, "r18": 18, "r204": 204}


def evaluated(engine, cfg, n):
    ps, seed, mix = program(cfg)
    assert ps.num_rules == RULES[cfg]
    corpus = K.Corpus(K.synth_resources(seed, n, mix=mix))
    assert corpus.n == n
    engine.evaluate_async(ps, corpus.upload(engine.device))
    v, _, _ = engine.fetch(ps, corpus)
    return ps, corpus, v


def host_select(v, sel):
    """The specification: cells with (sel[r] >> verdict) & 1, in row-major order."""
    hit = (sel[None, :].astype(np.uint32) >> v.astype(np.uint32)) & 1
    cells = np.flatnonzero(hit).astype(np.uint64)
    return cells, v.ravel()[cells.astype(np.int64)]


def selections(R):
    mix = np.where(np.arange(R) % 2 == 1, K.SEL(FAIL) | K.SEL(ERROR), K.SEL(PASS) | K.SEL(SKIP)).astype(np.uint8)
    return {"none": np.zeros(R, np.uint8), "all": np.full(R, 0xFF, np.uint8),
            "responses": np.full(R, K.SEL_RESPONSES, np.uint8), "mix": mix}


SHAPES = ([("r1", n) for n in (1, 15, 16, 17, 4095, 4096, 4097)] +
          [("r3", n) for n in (1, 5, 6, 64, 1365, 1366, 5000)] +
          [("r18", n) for n in (227, 228, 4096)] +
          [("r204", n) for n in (21, 2000, 20100)] +
          # 45000 x 204 = 2242 tiles and 2250 row groups: both persistent grids loop
          [("r204", 45000)])


@pytest.mark.parametrize("cfg,n", SHAPES, ids=[f"{c}-{n}" for c, n in SHAPES])
def test_select_and_summaries_match_host(engine, cfg, n):
    ps, corpus, v = evaluated(engine, cfg, n)
    R = ps.num_rules
    if n >= 64:  # a matrix worth reducing: matched and unmatched cells
        assert (v == 0).any() and (v != 0).any()
    for name, sel in selections(R).items():
        want_cells, want_v = host_select(v, sel)
        cells, verd, total = engine.select_cells(ps, corpus, sel)
        assert total == want_cells.size, (name, total, want_cells.size)
        assert cells.dtype == np.uint64 and verd.dtype == np.uint8
        assert np.array_equal(cells, want_cells), name
        assert np.array_equal(verd, want_v), name
        if name == "none":
            assert total == 0 and cells.size == 0
        if name == "all":  # nothing read past the end of the matrix, nothing dropped
            assert total == n * R and np.array_equal(cells, np.arange(n * R, dtype=np.uint64))
    # a scalar mask is broadcast to every rule; without the verdict array
    cells, verd, total = engine.select_cells(ps, corpus, K.SEL_RESPONSES, with_verdicts=False)
    assert np.array_equal(cells, host_select(v, np.full(R, K.SEL_RESPONSES, np.uint8))[0]) and verd.size == 0

    want = K.row_summaries(ps, v)
    got = engine.row_summaries(ps, corpus)
    assert got.shape == (n, 6) and got.dtype == np.uint16
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
    # windows: row0 > 0 up to the last row, an inner window, no rows, rows past the corpus
    for row0, nrows in ((n // 3, n - n // 3), (n // 2, min(7, n - n // 2)), (n - 1, 1)):
        assert np.array_equal(engine.row_summaries(ps, corpus, row0, nrows), want[row0:row0 + nrows]), (row0, nrows)
    assert engine.row_summaries(ps, corpus, n // 2, 0).shape == (0, 6)
    assert engine.row_summaries(ps, corpus, n, 0).shape == (0, 6)
    with pytest.raises(K.KpeError) as e:
        engine.row_summaries(ps, corpus, n // 2, n - n // 2 + 1)
    assert e.value.status == 1  # KPE_E_INVALID


def test_unscored_fail_counts_as_warn_on_device(engine):
    """The same corpus under a scored and an unscored copy of one policy: the device's fail
    column of the first is the warn column of the second."""
    (ps, _, _), (psu, _, _) = program("r3"), program("r3u")
    corpus = K.Corpus(K.synth_resources(0xC2, 777, mix=K.SYNTH_MIXED)).upload(engine.device)
    engine.evaluate_async(ps, corpus)
    a = engine.row_summaries(ps, corpus)
    engine.evaluate_async(psu, corpus)
    b = engine.row_summaries(psu, corpus)
    f, w = K.SUMMARY_FIELDS.index("fail"), K.SUMMARY_FIELDS.index("warn")
    assert a[:, f].sum() > 0 and a[:, w].sum() == 0
    assert b[:, f].sum() == 0 and np.array_equal(b[:, w], a[:, f])
    keep = [i for i in range(6) if i not in (f, w)]
    assert np.array_equal(a[:, keep], b[:, keep])


def test_cap_leaves_the_rest_untouched(engine):
    ps, corpus, v = evaluated(engine, "r3", 5000)
    R = ps.num_rules
    L = load()
    sel = np.full(R, K.SEL_RESPONSES, np.uint8)
    want_cells, want_v = host_select(v, sel)
    total = want_cells.size
    assert total > 100
    # count only
    assert L.kpe_select_cells(engine.device.h, ps.h, corpus.h, sel.ctypes.data, None, None, 0) == total
    cap = total // 2
    cells = np.full(total + 8, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    verd = np.full(total + 8, 0xA5, dtype=np.uint8)
    got = L.kpe_select_cells(engine.device.h, ps.h, corpus.h, sel.ctypes.data, cells.ctypes.data, verd.ctypes.data, cap)
    assert got == total
    assert np.array_equal(cells[:cap], want_cells[:cap]) and np.array_equal(verd[:cap], want_v[:cap])
    assert (cells[cap:] == np.uint64(0xDEADBEEFDEADBEEF)).all() and (verd[cap:] == 0xA5).all()
    # a generous cap: everything, and only that, is written
    cells[:] = np.uint64(0xDEADBEEFDEADBEEF)
    got = L.kpe_select_cells(engine.device.h, ps.h, corpus.h, sel.ctypes.data, cells.ctypes.data, None, 1 << 40)
    assert got == total and np.array_equal(cells[:total], want_cells)
    assert (cells[total:] == np.uint64(0xDEADBEEFDEADBEEF)).all()
    # the binding: cap through Engine.select_cells
    c2, v2, t2 = engine.select_cells(ps, corpus, sel, cap=cap)
    assert t2 == total and np.array_equal(c2, want_cells[:cap]) and np.array_equal(v2, want_v[:cap])


def test_selected_cells_feed_pattern_traces(engine):
    """select_cells' FAIL cells of the pattern rules, passed unchanged to pattern_traces, give the
    records of the list a host walk of the matrix builds."""
    ps = K.PolicySet(c5_policy_set())
    corpus = K.Corpus(K.synth_resources(0xC5, 300, mix=K.SYNTH_FANOUT))
    v, _, _ = engine.evaluate(ps, corpus)
    sel = np.array([0 if pss else K.SEL(FAIL) for pss in ps.is_pss], dtype=np.uint8)
    assert sel.any()
    host_cells, _ = host_select(v, sel)
    assert host_cells.size > 0
    cells, verd, total = engine.select_cells(ps, corpus, sel)
    assert total == host_cells.size and np.array_equal(cells, host_cells) and (verd == FAIL).all()
    got = engine.pattern_traces(ps, corpus, cells)
    want = engine.pattern_traces(ps, corpus, host_cells)
    assert np.array_equal(got, want)
    assert (got[:, 0, 0] & 0x1000000).all()  # KPE_TR_VALID: every selected cell has a record


def test_queries_need_an_evaluation(engine):
    ps, seed, mix = program("r3")
    corpus = K.Corpus(K.synth_resources(seed, 64, mix=mix)).upload(engine.device)
    for q in (lambda: engine.select_cells(ps, corpus, K.SEL_RESPONSES), lambda: engine.row_summaries(ps, corpus)):
        with pytest.raises(K.KpeError) as e:
            q()
        assert e.value.status == 5  # KPE_E_STATE
    # evaluated with another program: still no evaluation of this one
    other, _, _ = program("r3u")
    engine.evaluate_async(other, corpus)
    engine.device.sync()
    for q in (lambda: engine.select_cells(ps, corpus, K.SEL_RESPONSES), lambda: engine.row_summaries(ps, corpus)):
        with pytest.raises(K.KpeError) as e:
            q()
        assert e.value.status == 5
    assert engine.select_cells(other, corpus, K.SEL_RESPONSES)[2] > 0
