"""Per-namespace rule counts on the device (kpe_fetch_namespace_counts) against the host fold
(kpe_namespace_counts_host) over the matrix kpe_fetch returns, with exact equality. The matrix
itself is pinned to the oracle by the parity suites; these tests pin the reduction to the matrix.

Shapes: the smallest at which each mechanism can go wrong. The kernels take work items of at most
512 rows of one namespace (kNsChunk: 512 rows are one item whose counters are stored, 513 two items
that add atomically) on at most 2048 persistent blocks (kNsGrid: 5000 one-row namespaces make the
grid loop). R < 16 (kNsNarrow) takes the one-row-per-lane kernel (r1, r3). From 16 rules a lane owns
a unit of the row: one column (r18, r207, r411), or four when R is a multiple of 4 (r204, r408: a
word of four NA cells is passed over). Up to 128 units (kNsLdsUnits) the block's row slices are
summed in LDS (r18, r204, r408); past that a lane's registers go straight to memory (r207), in
tiles of 256 units (r411: two tiles). A lane keeps 8 row loads in flight (kNsBatch): r204-21 has
only the loop's tail, the 512-row items whole batches and a tail."""
import copy
import functools
import json
import re

import numpy as np
import pytest

import kyverno_amd as K
from kyverno_amd._lib import load
from tests.policies import c3_policy_set, parity_policy_set, restricted_latest, selector_policy

pytestmark = pytest.mark.gpu

UNSCORED = {"policies.kyverno.io/scored": "false"}
SENTINEL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def engine():
    return K.Engine(ordinal=0)


def _unscored(pols, which):
    pols = copy.deepcopy(pols)
    for i in which:
        pols[i]["metadata"].setdefault("annotations", {}).update(UNSCORED)
    return pols


def _renamed(pols, suffix):
    pols = copy.deepcopy(pols)
    for p in pols:
        p["metadata"]["name"] += suffix
    return pols


@functools.lru_cache(maxsize=None)
def program(cfg):
    """(PolicySet, synth seed, synth mix) of a shape's program: the shapes of test_gpu_select.py
    (some policies unscored: the table counts raw codes, so their fails stay fails), and wider
    ones for the kernel's paths past 128 and 256 column units."""
    if cfg == "r1":  # selectors disable autogen: one rule
        return K.PolicySet([selector_policy("wild-both", selector={"matchLabels": {"*": "*"}})]), 0xC4, K.SYNTH_SELECTORS
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
    if cfg == "r207":
        return K.PolicySet(c3_policy_set() + [restricted_latest()]), 0xC3, K.SYNTH_C3
    if cfg == "r408":
        return K.PolicySet(c3_policy_set() + _renamed(c3_policy_set(), "-b")), 0xC3, K.SYNTH_C3
    if cfg == "r411":
        return K.PolicySet(c3_policy_set() + _renamed(c3_policy_set(), "-b") + [restricted_latest()]), 0xC3, K.SYNTH_C3
    raise KeyError(cfg)


RULES = {"r1": 1, "r3": 3, "r3u": 3, "r18": 18, "r204": 204, "r207": 207, "r408": 408, "r411": 411}


def relayout(nd, layout):
    """The corpus's lines under a namespace layout."""
    if layout == "generated":
        return nd
    docs = [json.loads(x) for x in nd.split(b"\n") if x.strip()]
    rng = np.random.RandomState(len(docs))
    if layout == "random1000":  # 1000 namespaces in random order
        for d, k in zip(docs, rng.randint(0, 1000, len(docs))):
            d["metadata"]["namespace"] = f"ns-{k:04d}"
    elif layout == "sorted":
        docs.sort(key=lambda d: d["metadata"].get("namespace", ""))
    elif layout == "one":  # a few hot counters for every block
        for d in docs:
            d["metadata"]["namespace"] = "only"
    elif layout == "own":  # G = N
        for i, d in enumerate(docs):
            d["metadata"]["namespace"] = f"own-{i}"
    elif layout == "tenth-missing":
        for d in docs[::10]:
            d["metadata"].pop("namespace", None)
    else:
        raise KeyError(layout)
    return "\n".join(json.dumps(d, separators=(",", ":")) for d in docs).encode()


def evaluated(engine, cfg, n, layout="generated"):
    ps, seed, mix = program(cfg)
    assert ps.num_rules == RULES[cfg]
    corpus = K.Corpus(relayout(K.synth_resources(seed, n, mix=mix), layout))
    assert corpus.n == n
    engine.evaluate_async(ps, corpus.upload(engine.device))
    v, _, cnt = engine.fetch(ps, corpus)
    return ps, corpus, v, cnt


def check_table(engine, ps, corpus, v, cnt):
    """Every assertion of one evaluated (program, corpus): the whole table, its sums, windows,
    sentinels past a window, and a second call."""
    L = load()
    n, R, G = corpus.n, ps.num_rules, len(corpus.namespaces)
    want = K.namespace_counts(ps, corpus, v)  # the specification: the host fold of the fetched matrix
    got = engine.namespace_counts(ps, corpus)
    assert got.shape == (G, R, 6) and got.dtype == np.uint32
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
    # summed over the groups: the per-rule kpe_counts of fetch
    tot = got.sum(axis=0, dtype=np.uint64)
    for r in range(R):
        assert dict(zip(K.NS_COUNT_FIELDS, (int(x) for x in tot[r]))) == {k: cnt[r][k] for k in K.NS_COUNT_FIELDS}, r
    # the six counters plus the derived NA: the group's rows
    row_ns = corpus.row_namespaces()
    na = np.zeros((G, R), dtype=np.int64)
    np.add.at(na, row_ns, (v == 0).astype(np.int64))
    assert np.array_equal(got.sum(axis=2, dtype=np.int64) + na,
                          np.broadcast_to(corpus.namespace_rows().astype(np.int64)[:, None], (G, R)))
    # a second call: the cached index, and nothing accumulated across calls
    assert np.array_equal(engine.namespace_counts(ps, corpus), got)
    # windows: g0 > 0 to the end, an inner window of 3 groups, the last group alone, no group
    for g0, ng in ((G // 3, G - G // 3), (G // 2, min(3, G - G // 2)), (G - 1, 1)):
        assert np.array_equal(engine.namespace_counts(ps, corpus, g0, ng), want[g0:g0 + ng]), (g0, ng)
    assert np.array_equal(engine.namespace_counts(ps, corpus, G // 3), want[G // 3:])
    assert engine.namespace_counts(ps, corpus, G // 2, 0).shape == (0, R, 6)
    assert engine.namespace_counts(ps, corpus, G, 0).shape == (0, R, 6)
    with pytest.raises(K.KpeError) as e:
        engine.namespace_counts(ps, corpus, G // 2, G - G // 2 + 1)
    assert e.value.status == 1  # KPE_E_INVALID
    # memory past the window stays untouched
    g0, ng = G // 2, min(3, G - G // 2)
    buf = np.full((ng + 2, R, 6), SENTINEL, dtype=np.uint32)
    assert L.kpe_fetch_namespace_counts(engine.device.h, ps.h, corpus.h, g0, ng, buf.ctypes.data) == 0
    assert np.array_equal(buf[:ng], want[g0:g0 + ng]) and (buf[ng:] == SENTINEL).all()
    assert L.kpe_fetch_namespace_counts(engine.device.h, ps.h, corpus.h, g0, 0, buf.ctypes.data) == 0
    assert np.array_equal(buf[:ng], want[g0:g0 + ng]) and (buf[ng:] == SENTINEL).all()
    return got


SHAPES = ([("r1", n) for n in (1, 17, 4097)] +
          [("r3", n) for n in (1, 64, 65)] +
          [("r18", 4096)] +
          [("r204", n) for n in (21, 20100, 45000)] +
          [("r207", 700), ("r408", 700), ("r411", 700)])


@pytest.mark.parametrize("cfg,n", SHAPES, ids=[f"{c}-{n}" for c, n in SHAPES])
def test_counts_match_host_fold(engine, cfg, n):
    ps, corpus, v, cnt = evaluated(engine, cfg, n)
    if n >= 64:  # a matrix worth reducing: matched and unmatched cells
        assert (v == 0).any() and (v != 0).any()
    check_table(engine, ps, corpus, v, cnt)


LAYOUTS = ([("r3", 5000, lay) for lay in ("generated", "random1000", "sorted", "one", "own", "tenth-missing")] +
           [("r204", 20100, lay) for lay in ("sorted", "one", "tenth-missing")] +
           [("r204", 5000, "own")] +
           # one namespace of exactly one work item, and of one row more
           [(cfg, n, "one") for cfg in ("r3", "r18", "r204", "r207") for n in (512, 513)])


@pytest.mark.parametrize("cfg,n,layout", LAYOUTS, ids=[f"{c}-{n}-{lay}" for c, n, lay in LAYOUTS])
def test_namespace_layouts(engine, cfg, n, layout):
    ps, corpus, v, cnt = evaluated(engine, cfg, n, layout)
    G = len(corpus.namespaces)
    rows = corpus.namespace_rows()
    if layout == "one":
        assert int(rows.max()) == n  # "only"; "" has no rows
    if layout == "own":
        assert G == n + 1 and rows.max() == 1
    if layout == "random1000":
        assert G >= 990
    if layout == "tenth-missing":
        assert rows[corpus.namespaces.index("")] >= n // 10
    got = check_table(engine, ps, corpus, v, cnt)
    assert got.any()


def test_raw_codes_whether_scored_or_not(engine):
    """The same corpus under a scored and an unscored copy of one policy: the same table (the
    scored fold is the consumer's, kpe_cli_summary_ns)."""
    (ps, _, _), (psu, _, _) = program("r3"), program("r3u")
    corpus = K.Corpus(K.synth_resources(0xC2, 777, mix=K.SYNTH_MIXED)).upload(engine.device)
    engine.evaluate_async(ps, corpus)
    a = engine.namespace_counts(ps, corpus)
    engine.evaluate_async(psu, corpus)
    b = engine.namespace_counts(psu, corpus)
    f, w = K.NS_COUNT_FIELDS.index("fail"), K.NS_COUNT_FIELDS.index("warn")
    assert a[:, :, f].sum() > 0 and a[:, :, w].sum() == 0 and np.array_equal(a, b)


def test_needs_an_evaluation(engine):
    ps, seed, mix = program("r3")
    corpus = K.Corpus(K.synth_resources(seed, 64, mix=mix))
    with pytest.raises(K.KpeError) as e:  # not uploaded
        engine.namespace_counts(ps, corpus)
    assert e.value.status == 5  # KPE_E_STATE
    corpus.upload(engine.device)
    with pytest.raises(K.KpeError) as e:
        engine.namespace_counts(ps, corpus)
    assert e.value.status == 5
    # evaluated with another program: still no evaluation of this one
    other, _, _ = program("r3u")
    engine.evaluate_async(other, corpus)
    engine.device.sync()
    with pytest.raises(K.KpeError) as e:
        engine.namespace_counts(ps, corpus)
    assert e.value.status == 5
    assert engine.namespace_counts(other, corpus).any()


def test_batch_of_resident_shards(engine):
    ps, seed, mix = program("r3")
    nd = K.synth_resources(seed, 3000, mix=mix)
    lines = nd.split(b"\n")
    shards = [K.Corpus(b"\n".join(part)).upload(engine.device) for part in (lines[:1300], lines[1300:3000])]
    assert [s.n for s in shards] == [1300, 1700]
    engine.evaluate_batch_async(ps, shards)
    tables = [engine.namespace_counts(ps, s) for s in shards]
    for s, t in zip(shards, tables):
        v, _, _ = engine.fetch(ps, s)
        assert np.array_equal(t, K.namespace_counts(ps, s, v)) and t.any()
    # merged by name: the table of the whole corpus
    from kyverno_amd.shard import merge_namespace_counts

    whole = K.Corpus(nd)
    v, _, _ = engine.evaluate(ps, whole)
    names, merged = merge_namespace_counts([(s.namespaces, t) for s, t in zip(shards, tables)])
    want = dict(zip(whole.namespaces, K.namespace_counts(ps, whole, v)))
    for nm, tab in zip(names, merged):
        assert np.array_equal(tab, want[nm].astype(np.uint64)), nm
    assert {nm for nm, t in want.items() if t.any()} <= set(names)


def test_cli_summary_with_overrides_end_to_end(engine, oracle):
    """An Audit policy with an Enforce override on team-*-prod over SYNTH_C3: the totals from the
    device's table equal those from the host table of the oracle's matrix, and --audit-warn moves
    them away from the totals without the override."""
    base = copy.deepcopy(parity_policy_set()[0])
    base["spec"]["validationFailureAction"] = "Audit"
    pol = copy.deepcopy(base)
    pol["spec"]["validationFailureActionOverrides"] = [{"action": "Enforce", "namespaces": ["team-*-prod"]}]
    nd = K.synth_resources(0xC3, 2000, mix=K.SYNTH_C3)
    assert re.search(rb'"namespace":"team-\d+-prod"', nd)
    ps, ps_base = K.PolicySet([pol]), K.PolicySet([base])
    ref = oracle.validate([pol], nd, nthreads=8)
    corpus = K.Corpus(nd)
    engine.evaluate_async(ps, corpus.upload(engine.device))
    dev_table = engine.namespace_counts(ps, corpus)
    host_table = K.namespace_counts(ps, corpus, ref)
    assert np.array_equal(dev_table, host_table)
    for aw in (False, True):
        want = K.cli_summary_ns(ps, corpus, host_table, aw)
        assert K.cli_summary_ns(ps, corpus, dev_table, aw) == want
        plain = K.cli_summary_ns(ps_base, corpus, host_table, aw)
        assert (want != plain) == aw
    assert K.cli_summary_ns(ps, corpus, dev_table, True)["fail"] > 0
