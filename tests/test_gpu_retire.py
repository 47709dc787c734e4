"""Retired rows on the device (kpe_corpus_retire_rows): from the next evaluation on a retired row
gives no response, whatever it would otherwise be, in every form of evaluation and to every consumer.

The corpus is synth_resources(seed, 4096, mix=2) plus 193 further rows (4289: a partial last tile of
64), among them a row past an encoding limit (256 containers: every cell KPE_UNDECIDED), a row with
a decode error (KPE_ERROR cells) and a row with a context error (an invalid image reference: every
cell KPE_UNDECIDED). The expectation is the oracle's matrix (the limit row at KPE_UNDECIDED, as the
device leaves it to the reference engine) with the retired rows zeroed. Retired sets: the first row,
the tile edges and the last row, the three flagged rows, 255 / 256 / 257 rows at a stride (the retire
pass takes 256 work items per block), and every row. A retired set only grows, so each case flattens
its own corpus; the oracle's matrix is computed once per program and shared."""
import ctypes
import functools
import json

import numpy as np
import pytest

import kyverno_amd as K
from kyverno_amd._lib import load
from tests.policies import _golden, pss_policy, restricted_latest
from tests.test_gpu_lean_shapes import BATCHED, LEAN6, stats_of

pytestmark = pytest.mark.gpu

UNDECIDED, ERROR = 7, 4
NO_AUTOGEN = {"pod-policies.kyverno.io/autogen-controllers": "none"}


def _pod(name, **kw):
    p = {"apiVersion": "v1", "kind": "Pod", "metadata": {"name": name, "namespace": "ns-0001"},
         "spec": {"containers": [{"name": "c", "image": "nginx:1.25"}]}}
    p["spec"].update(kw)
    return p


@functools.lru_cache(maxsize=None)
def corpus_ndjson():
    """(NDJSON, N, {"limit", "decode", "context": row})."""
    base = K.synth_resources(0xD1, 4096, mix=2).strip(b"\n")
    extra = K.synth_resources(0xD2, 190, mix=2).strip(b"\n").split(b"\n")
    assert len(extra) == 190 and base.count(b"\n") == 4095
    flagged = {"limit": 4096 + 17, "decode": 4096 + 64, "context": 4096 + 150}
    rows = {"limit": _pod("many", containers=[{"name": f"c{j}", "image": "x"} for j in range(256)]),
            "decode": _pod("decode", containers=[{"name": "c", "image": "nginx", "readinessProbe": {"periodSeconds": "3"}}]),
            "context": _pod("context", containers=[{"name": "c", "image": "Nginx"}])}
    for what in ("limit", "decode", "context"):
        extra.insert(flagged[what] - 4096, json.dumps(rows[what], separators=(",", ":")).encode())
    nd = base + b"\n" + b"\n".join(extra)
    n = 4096 + 193
    assert nd.count(b"\n") + 1 == n
    flags = K.Corpus(nd).row_flags()
    assert flags[flagged["limit"]] & 2 and flags[flagged["decode"]] & 1 and flags[flagged["context"]] & 8
    return nd, n, flagged


def retired_sets():
    _, n, fl = corpus_ndjson()
    return {"first": [0], "tile-edges": [63, 64, 65, 127, 128, n - 1], "flagged": sorted(fl.values()),
            "255": list(range(3, 3 + 255 * 16, 16)), "256": list(range(5, 5 + 256 * 16, 16)),
            "257": list(range(n - 1, n - 1 - 257 * 16, -16)), "all": list(range(n))}


SETS = ["first", "tile-edges", "flagged", "255", "256", "257", "all"]
LEAN_PROGRAMS = ["r1", "r3", "r5"]
PROGRAMS = LEAN_PROGRAMS + ["chart", "pssx", "one"]


@functools.lru_cache(maxsize=None)
def program(name):
    if name == "r1":  # one kind-only podSecurity rule
        p = restricted_latest()
        p["metadata"]["annotations"] = dict(NO_AUTOGEN)
        pols = [p]
    elif name == "r3":  # restricted:latest with its autogen rules: the packed-row store
        pols = [restricted_latest()]
    elif name == "r5":  # five podSecurity rules of one policy
        p = pss_policy("five", "baseline", "latest")
        p["metadata"]["annotations"] = dict(NO_AUTOGEN)
        for k, (lvl, ver) in enumerate([("restricted", "latest"), ("baseline", "v1.19"), ("restricted", "v1.24"),
                                        ("privileged", "latest")]):
            p["spec"]["rules"].append({"name": f"five-{k}", "match": {"any": [{"resources": {"kinds": ["Pod"]}}]},
                                       "validate": {"podSecurity": {"level": lvl, "version": ver}}})
        pols = [p]
    elif name == "chart":  # the chart's pattern, deny and foreach rules
        chart = _golden("chart_policies.json")
        pols = chart["baseline"] + chart["restricted"]
    elif name == "pssx":  # podSecurity rules with exclusions
        pols = [pss_policy("x-caps", "baseline", exclude=[{"controlName": "Capabilities", "images": ["*"]}]),
                pss_policy("x-host", "restricted", "v1.24", exclude=[{"controlName": "Host Namespaces"},
                                                                      {"controlName": "HostPath Volumes"}])]
    elif name == "one":  # applyRules: One over two rules
        p = pss_policy("one", "baseline", "latest", apply_one=True)
        p["spec"]["rules"].append({"name": "second", "match": {"any": [{"resources": {"kinds": ["Pod"]}}]},
                                   "validate": {"podSecurity": {"level": "restricted", "version": "latest"}}})
        pols = [p, restricted_latest()]
    else:
        raise KeyError(name)
    ps = K.PolicySet(pols)
    want = {"r1": 1, "r3": 3, "r5": 5}.get(name)
    assert want is None or ps.num_rules == want
    return pols, ps


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's matrix of the whole corpus with nothing retired; the limit row is the device's to
    leave undecided."""
    from tests import oracle_lib

    nd, n, fl = corpus_ndjson()
    pols, ps = program(name)
    ref = oracle_lib.load().validate(pols, nd, nthreads=8).copy()
    assert ref.shape == (n, ps.num_rules)
    ref[fl["limit"]] = UNDECIDED
    assert (ref[fl["context"]] == UNDECIDED).all()
    ref.setflags(write=False)
    return ref


def expected(name, rows):
    want = reference(name).copy()
    want[np.asarray(rows, dtype=np.int64)] = 0
    return want


@pytest.fixture(scope="module")
def engine():
    return K.Engine(ordinal=0)


def new_corpus(engine, retire=None, before_upload=False):
    nd, n, _ = corpus_ndjson()
    c = K.Corpus(nd)
    assert c.n == n
    if retire is not None and before_upload:
        engine.retire_rows(c, retire)  # recorded on the host: travels with the upload
    c.upload(engine.device)
    if retire is not None and not before_upload:
        engine.retire_rows(c, retire)
    return c


def histogram(v):
    keys = {"na": 0, "pass": 1, "fail": 2, "warn": 3, "error": 4, "skip": 5, "undecided": 7}
    return [{k: int((v[:, r] == code).sum()) for k, code in keys.items()} for r in range(v.shape[1])]


@pytest.fixture(scope="module")
def plain_masks(engine):
    """The mask words of a corpus with nothing retired, per program (fetched once)."""
    cache = {}

    def get(name):
        if name not in cache:
            _, ps = program(name)
            c = new_corpus(engine)
            v, m, _ = engine.evaluate(ps, c, check_masks=True)
            assert np.array_equal(v, reference(name)), int((v != reference(name)).sum())
            cache[name] = engine.cv_masks(ps, c, raw=True)
        return cache[name]

    return get


@pytest.mark.parametrize("rset", SETS)
@pytest.mark.parametrize("name", PROGRAMS)
def test_retired_rows_give_no_response(engine, plain_masks, name, rset):
    _, ps = program(name)
    rows = retired_sets()[rset]
    want = expected(name, rows)
    c = new_corpus(engine, rows, before_upload=(rset in ("first", "256")))
    assert engine.retired_rows(c).tolist() == sorted(rows)
    # kpe_evaluate, without masks
    v, _, cnt = engine.evaluate(ps, c)
    assert np.array_equal(v, want), np.argwhere(v != want)[:5].tolist()
    assert cnt == histogram(want)
    # kpe_evaluate_async_ex with masks, then the fetches
    engine.evaluate_async(ps, c, masks=True)
    v, _, cnt = engine.fetch(ps, c)
    m = engine.cv_masks(ps, c, raw=True)
    assert np.array_equal(v, want) and cnt == histogram(want)
    want_m = plain_masks(name).copy()
    want_m[np.asarray(rows, dtype=np.int64)] = 0
    assert not m[np.asarray(rows, dtype=np.int64)].any() and np.array_equal(m, want_m)
    # a cold evaluation rebuilds the prologue; the retired rows stay retired
    engine.evaluate_async(ps, c, cold=True)
    assert np.array_equal(engine.fetch(ps, c)[0], want)
    if name in LEAN_PROGRAMS and rset == "tile-edges":
        assert load().kpe_debug_lean_kind(c.h, 0) == LEAN6
        st = stats_of(engine, lambda: engine.evaluate_async(ps, c))
        assert st.scan_kernel == LEAN6 and load().kpe_debug_lean_form(engine.device.h) >= 0, st.scan_kernel


@pytest.mark.parametrize("masks", [False, True], ids=["verdicts", "masks"])
@pytest.mark.parametrize("name", LEAN_PROGRAMS)
def test_batch_mixes_retired_and_plain_corpora(engine, plain_masks, name, masks):
    """kpe_evaluate_batch_async over [c_retired, c_plain, c_retired]: the corpus with a limit row is
    launched on its own; the 4096 synthetic rows alone ride in one multi-shard LEAN launch, whose
    retired shards get their pass behind it."""
    _, ps = program(name)
    rows = retired_sets()["tile-edges"]
    c_ret, c_plain = new_corpus(engine, rows), new_corpus(engine)
    engine.evaluate_batch_async(ps, [c_ret, c_plain, c_ret], masks=masks)
    for c, want in ((c_ret, expected(name, rows)), (c_plain, reference(name))):
        v, _, cnt = engine.fetch(ps, c)
        assert np.array_equal(v, want) and cnt == histogram(want)
    if masks:
        want_m = plain_masks(name).copy()
        assert np.array_equal(engine.cv_masks(ps, c_plain, raw=True), want_m)
        want_m[np.asarray(rows, dtype=np.int64)] = 0
        assert np.array_equal(engine.cv_masks(ps, c_ret, raw=True), want_m)
    # the multi-shard launch: no limit row
    nd = K.synth_resources(0xD1, 4096, mix=2)
    rows = [r for r in rows if r < 4096] + [4095]
    a, b, p = K.Corpus(nd).upload(engine.device), K.Corpus(nd).upload(engine.device), K.Corpus(nd).upload(engine.device)
    engine.retire_rows(a, rows)
    engine.retire_rows(b, [0, 4000])
    for c in (a, p, b):
        engine.evaluate(ps, c, check_masks=masks)  # binds: the next batch is one launch
    st = stats_of(engine, lambda: engine.evaluate_batch_async(ps, [a, p, b, a], masks=masks))
    assert st.launches == 1 and st.scan_kernel == BATCHED and load().kpe_debug_lean_form(engine.device.h) >= 0
    ref = reference(name)[:4096]
    for c, rr in ((a, rows), (p, []), (b, [0, 4000])):
        want = ref.copy()
        want[rr] = 0
        v, _, cnt = engine.fetch(ps, c)
        assert np.array_equal(v, want) and cnt == histogram(want)
        if masks:
            m = engine.cv_masks(ps, c, raw=True)
            assert not m[rr].any() and np.array_equal(np.delete(m, rr, axis=0), np.delete(plain_masks(name)[:4096], rr, axis=0))


@pytest.mark.parametrize("name", ["r3", "chart", "one"])
def test_every_consumer_sees_the_retired_rows(engine, name):
    """Each sparse fetch against its host twin over the expected matrix."""
    _, ps = program(name)
    _, n, fl = corpus_ndjson()
    R = ps.num_rules
    first = sorted(set(retired_sets()["tile-edges"]) | set(fl.values()))
    c = new_corpus(engine, first)
    want1 = expected(name, first)
    engine.evaluate_async(ps, c, masks=True)
    cells, verd, total = engine.select_cells(ps, c, K.SEL_RESPONSES)
    flat = want1.reshape(-1)
    assert total == int((flat != 0).sum()) and np.array_equal(cells, np.flatnonzero(flat).astype(np.uint64))
    assert np.array_equal(verd, flat[flat != 0])
    assert np.array_equal(engine.row_summaries(ps, c), K.row_summaries(ps, want1))
    assert not engine.row_summaries(ps, c, first[0], 1).any()
    assert np.array_equal(engine.namespace_counts(ps, c), K.namespace_counts(ps, c, want1))
    # retired rows still count as rows of their namespace: NA cells = rows - counters
    nsr = c.namespace_rows()
    assert int(nsr.sum()) == n
    ns = c.row_namespaces()
    na = np.stack([np.bincount(ns, weights=(want1[:, r] == 0), minlength=nsr.size) for r in range(R)], axis=1)
    assert np.array_equal(nsr[:, None] - engine.namespace_counts(ps, c).sum(axis=2), na.astype(np.uint64))
    salts = K.rule_salts(ps)
    for masks in (False, True):
        fp = engine.row_fingerprints(ps, c, masks=masks)
        mw = engine.cv_masks(ps, c, raw=True) if masks else None
        assert np.array_equal(fp, K.row_fingerprints(want1, salts, cv_masks=mw))
        assert not fp[first].any() and fp.any()  # "no report"
    sp = engine.fetch_report_rows(ps, c, first + [1, 2])
    assert not sp["verdict_rows"][:len(first)].any() and np.array_equal(sp["verdict_rows"][len(first):], want1[[1, 2]])
    assert all((np.asarray(sp[k]) // R >= len(first)).all() for k in ("mask_cells", "cond_cells", "pattern_cells"))
    ptr, nb = engine.device_verdicts(ps, c)
    assert nb == n * R
    # kept results and deltas: keep, retire more, evaluate again
    engine.keep_results(ps, c)
    engine.keep_fingerprints(ps, c)
    more = retired_sets()["255"]
    engine.retire_rows(c, more)
    # retiring after an evaluation changes nothing until the next one
    assert np.array_equal(engine.fetch(ps, c)[0], want1)
    assert engine.changed_rows(ps, c)[2] == 0 and engine.changed_rows_fp(ps, c)[3] == 0
    engine.evaluate_async(ps, c, masks=True)
    both = sorted(set(first) | set(more))
    assert engine.retired_rows(c).tolist() == both
    want2 = expected(name, both)
    assert np.array_equal(engine.fetch(ps, c)[0], want2)
    ident = np.arange(R, dtype=np.int32)
    wr, wv, wt = K.changed_rows(want1, want2, ident)
    rows, vr, total = engine.changed_rows(ps, c)
    assert total == wt > 0 and np.array_equal(rows, wr) and np.array_equal(vr, wv) and not vr.any()
    assert np.array_equal(engine.delta_transitions(ps, c), K.delta_transitions(want1, want2, ident))
    rows, _, fps, total = engine.changed_rows_fp(ps, c)
    assert np.array_equal(rows, wr) and not fps.any()
    # the packed exchange
    hip = ctypes.CDLL("libamdhip64.so")
    words = K.packed_words(n * R)
    buf, host = ctypes.c_void_p(), np.zeros(words, dtype=np.uint32)
    assert hip.hipMalloc(ctypes.byref(buf), ctypes.c_size_t(words * 4)) == 0
    try:
        engine.pack_verdicts(ps, c, buf.value, words)
        assert hip.hipMemcpy(ctypes.c_void_p(host.ctypes.data), buf, ctypes.c_size_t(words * 4), 2) == 0  # device to host
    finally:
        hip.hipFree(buf)
    assert np.array_equal(K.unpack_verdicts(host, n, R), want2)


def test_reupload_keeps_the_set_and_wrong_devices_are_refused(engine):
    _, ps = program("r3")
    _, n, _ = corpus_ndjson()
    rows = retired_sets()["257"]
    c = new_corpus(engine, rows)
    want = expected("r3", rows)
    assert np.array_equal(engine.evaluate(ps, c)[0], want)
    c.upload(engine.device)  # a new device copy: the set is sent again
    assert engine.retired_rows(c).tolist() == sorted(rows)
    assert np.array_equal(engine.evaluate(ps, c)[0], want)
    engine.retire_rows(c, [1])
    want[1] = 0
    assert np.array_equal(engine.evaluate(ps, c)[0], want)
    # an uploaded corpus: its own device, or KPE_E_STATE; a row >= N is KPE_E_INVALID; the set stays
    L = load()
    r = np.array([2], dtype=np.uint64)
    assert L.kpe_corpus_retire_rows(None, c.h, r.ctypes.data, 1) == 5
    r[0] = n
    assert L.kpe_corpus_retire_rows(engine.device.h, c.h, r.ctypes.data, 1) == 1
    assert engine.retired_rows(c).tolist() == sorted(rows + [1])
    assert np.array_equal(engine.evaluate(ps, c)[0], want)


def test_sharded_evaluation_retires_too(engine):
    _, ps = program("r3")
    rows = retired_sets()["tile-edges"]
    c = new_corpus(engine, rows)
    v, cnt = K.evaluate_sharded([engine], ps, [c])
    want = expected("r3", rows)
    assert np.array_equal(v, want) and cnt == histogram(want)
