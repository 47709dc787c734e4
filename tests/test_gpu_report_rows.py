"""Reports for a row list on the device: kpe_fetch_report_rows' three sparse lists and verdict rows
equal the host twin (kpe_report_cells_host) over the dense kpe_fetch / kpe_fetch_cv_masks /
kpe_fetch_cond_traces_ex rows, its pattern records equal kpe_pattern_traces over the absolute cells,
at every cap; Engine.report_rows equals the per-row renderer; ResidentScanner(reports=True) renders
the changed rows of an edit; and kpe_pattern_traces over a mixed list of foreach and plain cells
equals the same cells asked one by one (the guard of its one-gather form)."""
import ctypes
import json

import numpy as np
import pytest

import kyverno_amd as K
from kyverno_amd._lib import load
from kyverno_amd.engine import CTRACE_WORDS, RR_COND, RR_MASKS, RR_PATTERNS, TRACE_ROOTS, TRACE_WORDS, ReportRows
from tests.policies import cond_message_policy_set, foreach_message_policy_set, restricted_latest, selector_policy

pytestmark = pytest.mark.gpu

KPE_E_INVALID, KPE_E_STATE = 1, 5
FAIL, ERROR = 2, 4
ALL = RR_MASKS | RR_COND | RR_PATTERNS
REC = TRACE_ROOTS * TRACE_WORDS
S64, S32 = np.uint64(0xA5A5A5A5A5A5A5A5), np.uint32(0xA5A5A5A5)


@pytest.fixture(scope="module")
def engine():
    return K.Engine(ordinal=0)


def large_policies():
    from tests.test_gpu_pattern import chart_pattern_policies

    return chart_pattern_policies() + foreach_message_policy_set() + cond_message_policy_set()


def case_inputs(name, N):
    """(PolicySet, ndjson) of a program over N resources."""
    if name == "exception":
        from tests.pss_fuzz import exception_case

        pols, excs, nd = exception_case(41, npods=N)
        return K.PolicySet(pols, excs), nd
    nd = K.synth_resources(0x52 + N, N, mix=2)
    if name == "restricted":
        return K.PolicySet([restricted_latest()]), nd
    if name == "selector":
        return K.PolicySet([selector_policy("one", kinds=("Deployment", "Pod"),
                                            selector={"matchExpressions": [{"key": "app", "operator": "Exists"}]})]), nd
    return K.PolicySet(large_policies()), nd


def row_lists(N):
    rng = np.random.default_rng(N)
    k = max(N // 20, 1)
    picks = rng.integers(0, N, size=k, dtype=np.uint64)
    return {"empty": np.zeros(0, dtype=np.uint64), "first": np.array([0], dtype=np.uint64),
            "last": np.array([N - 1], dtype=np.uint64), "all": np.arange(N, dtype=np.uint64),
            "reversed": np.arange(N, dtype=np.uint64)[::-1].copy(), "seventh": np.arange(0, N, 7, dtype=np.uint64),
            "random": np.concatenate([picks, picks[:max(k // 3, 1)]])}


def guarded(n, dtype, words=1):
    return np.full((n + 3) * words * np.dtype(dtype).itemsize, 0xA5, dtype=np.uint8).view(dtype)


def fetch_guarded(engine, ps, corpus, rows, caps, flags=ALL):
    """kpe_fetch_report_rows into arrays with a sentinel tail: (arrays, totals)."""
    cm, cc, cp = caps
    R = ps.num_rules
    a = {"v": guarded(rows.size * R, np.uint8), "mc": guarded(cm, np.uint64), "mw": guarded(cm, np.uint32),
         "cc": guarded(cc, np.uint64), "cw": guarded(cc, np.uint32, CTRACE_WORDS), "pc": guarded(cp, np.uint64),
         "pt": guarded(cp, np.uint32, REC)}
    io = ReportRows(a["v"].ctypes.data, a["mc"].ctypes.data if cm else None, a["mw"].ctypes.data if cm else None, cm,
                    a["cc"].ctypes.data if cc else None, a["cw"].ctypes.data if cc else None, cc,
                    a["pc"].ctypes.data if cp else None, a["pt"].ctypes.data if cp else None, cp, 77, 77, 77)
    rbuf = rows if rows.size else np.zeros(1, dtype=np.uint64)
    st = load().kpe_fetch_report_rows(engine.device.h, ps.h, corpus.h, rbuf.ctypes.data, rows.size, flags, ctypes.byref(io))
    assert st == 0, load().kpe_last_error()
    return a, (io.mask_total, io.cond_total, io.pattern_total)


CASES = [(p, n) for p in ("restricted", "selector", "large", "exception") for n in (1, 63, 65, 2500)]


@pytest.mark.parametrize("prog,N", CASES, ids=[f"{p}-n{n}" for p, n in CASES])
def test_sparse_arrays_equal_the_twin(engine, prog, N):
    ps, nd = case_inputs(prog, N)
    corpus = K.Corpus(nd)
    assert corpus.n == N
    R = ps.num_rules
    v, _, _ = engine.evaluate(ps, corpus, check_masks=True)
    raw = engine.cv_masks(ps, corpus, raw=True)
    cx = engine.cond_traces(ps, corpus, ex=True)
    seen = np.zeros(3, dtype=np.int64)
    for what, rows in row_lists(N).items():
        ri = rows.astype(np.int64)
        want = K.report_cells(ps, v[ri], raw[ri], cx[ri])
        got = engine.fetch_report_rows(ps, corpus, rows)
        assert np.array_equal(got["verdict_rows"], v[ri]), what
        for key in ("mask_cells", "mask_words", "cond_cells", "cond_words", "pattern_cells"):
            assert np.array_equal(got[key], want[key]), (what, key)
        for key in ("mask_total", "cond_total", "pattern_total"):
            assert got[key] == want[key], (what, key)
        cells = want["pattern_cells"].astype(np.int64)
        absolute = (ri[cells // R] * R + cells % R).astype(np.uint64) if cells.size else np.zeros(0, dtype=np.uint64)
        assert np.array_equal(got["pattern_traces"], engine.pattern_traces(ps, corpus, absolute)), what
        seen += [want["mask_total"], want["cond_total"], want["pattern_total"]]
        # one kind at a time: the others give total 0 and their arrays are not read
        only = engine.fetch_report_rows(ps, corpus, rows, masks=False, patterns=False)
        assert only["mask_total"] == 0 and only["pattern_total"] == 0
        assert np.array_equal(only["cond_cells"], want["cond_cells"]) and np.array_equal(only["cond_words"], want["cond_words"])
    if prog in ("restricted", "exception") and N >= 63:
        assert seen[0] > 0
    if prog == "exception" and N == 2500:
        assert (raw >> 31).any()  # KPE_CVM_XMATCH comes through
    if prog == "large" and N >= 63:
        assert seen[1] > 0 and seen[2] > 0
    # caps, over the densest list: count-only, exact, one short, zero against a non-zero total;
    # nothing past min(total, cap) is written
    rows = row_lists(N)["all"]
    ri = rows.astype(np.int64)
    want = K.report_cells(ps, v[ri], raw[ri], cx[ri])
    tot = (want["mask_total"], want["cond_total"], want["pattern_total"])
    absolute = want["pattern_cells"].astype(np.int64)
    rec = engine.pattern_traces(ps, corpus, absolute.astype(np.uint64))  # rows is the identity list
    for caps in ((0, 0, 0), tot, tuple(max(t - 1, 0) for t in tot), (0, tot[1], 0), (min(tot[0], 5), 0, min(tot[2], 70))):
        a, totals = fetch_guarded(engine, ps, corpus, rows, caps)
        assert tuple(totals) == tot, caps
        km, kc, kp = (min(t, c) for t, c in zip(tot, caps))
        assert np.array_equal(a["v"][:N * R], v.reshape(-1)) and (a["v"][N * R:] == 0xA5).all()
        assert np.array_equal(a["mc"][:km], want["mask_cells"][:km]) and (a["mc"][km:] == S64).all(), caps
        assert np.array_equal(a["mw"][:km], want["mask_words"][:km]) and (a["mw"][km:] == S32).all(), caps
        assert np.array_equal(a["cc"][:kc], want["cond_cells"][:kc]) and (a["cc"][kc:] == S64).all(), caps
        assert np.array_equal(a["cw"][:kc * 4], want["cond_words"][:kc].reshape(-1)) and (a["cw"][kc * 4:] == S32).all(), caps
        assert np.array_equal(a["pc"][:kp], want["pattern_cells"][:kp]) and (a["pc"][kp:] == S64).all(), caps
        assert np.array_equal(a["pt"][:kp * REC], rec[:kp].reshape(-1)) and (a["pt"][kp * REC:] == S32).all(), caps


def test_errors(engine):
    L = load()
    ps = K.PolicySet([restricted_latest()])
    corpus = K.Corpus(K.synth_resources(3, 65, mix=2))
    rows = np.array([0, 64, 3], dtype=np.uint64)
    io = ReportRows()
    corpus.upload(engine.device)
    # no evaluation of this program yet
    assert L.kpe_fetch_report_rows(engine.device.h, ps.h, corpus.h, rows.ctypes.data, 3, ALL, ctypes.byref(io)) == KPE_E_STATE
    engine.evaluate_async(ps, corpus)  # without masks
    assert L.kpe_fetch_report_rows(engine.device.h, ps.h, corpus.h, rows.ctypes.data, 3, RR_MASKS, ctypes.byref(io)) == KPE_E_STATE
    assert L.kpe_fetch_report_rows(engine.device.h, ps.h, corpus.h, rows.ctypes.data, 3, RR_COND | RR_PATTERNS,
                                   ctypes.byref(io)) == 0
    with pytest.raises(K.KpeError) as e:
        engine.fetch_report_rows(ps, corpus, rows)
    assert e.value.status == KPE_E_STATE
    engine.evaluate_async(ps, corpus, masks=True)
    assert L.kpe_fetch_report_rows(engine.device.h, ps.h, corpus.h, rows.ctypes.data, 3, ALL, ctypes.byref(io)) == 0
    bad = np.array([0, 65], dtype=np.uint64)  # a row past N
    assert L.kpe_fetch_report_rows(engine.device.h, ps.h, corpus.h, bad.ctypes.data, 2, ALL, ctypes.byref(io)) == KPE_E_INVALID
    assert L.kpe_fetch_report_rows(engine.device.h, ps.h, corpus.h, rows.ctypes.data, 3, 8, ctypes.byref(io)) == KPE_E_INVALID
    assert L.kpe_fetch_report_rows(engine.device.h, ps.h, corpus.h, None, 3, ALL, ctypes.byref(io)) == KPE_E_INVALID
    io.cond_cap = 4  # a cap without its arrays
    assert L.kpe_fetch_report_rows(engine.device.h, ps.h, corpus.h, rows.ctypes.data, 3, ALL, ctypes.byref(io)) == KPE_E_INVALID
    other = K.PolicySet([restricted_latest()])  # an equal program that was not evaluated
    io = ReportRows()
    assert L.kpe_fetch_report_rows(engine.device.h, other.h, corpus.h, rows.ctypes.data, 3, ALL, ctypes.byref(io)) == KPE_E_STATE


def per_row_reports(engine, ps, corpus, v, lines, rows):
    """The per-row path: one trace call and one render call per listed row."""
    raw = engine.cv_masks(ps, corpus, raw=True)
    cx = engine.cond_traces(ps, corpus, ex=True)
    return [K.report_results(ps, v[i], cv_mask_row=raw[i], resource=lines[i], traces=engine.row_traces(ps, corpus, i),
                             corpus=corpus, cond_traces=cx[i]) for i in rows]


def test_rendered_reports_equal_the_per_row_path(engine):
    ps = K.PolicySet(large_policies() + [restricted_latest()])
    nd = K.synth_resources(0x52 + 2500, 2500, mix=2)
    lines = [l for l in nd.split(b"\n") if l]
    corpus = K.Corpus(nd)
    v, _, _ = engine.evaluate(ps, corpus, check_masks=True)
    rng = np.random.default_rng(5)
    rows = np.concatenate([rng.permutation(2500), rng.integers(0, 2500, size=50)]).astype(np.uint64)
    got = engine.report_rows(ps, corpus, rows, resources=[lines[int(i)] for i in rows])
    want = per_row_reports(engine, ps, corpus, v, lines, [int(i) for i in rows])
    assert len(got) == len(want) == rows.size
    bad = [k for k in range(rows.size) if got[k] != want[k]]
    assert not bad, (len(bad), int(rows[bad[0]]), got[bad[0]], want[bad[0]])
    msgs = [r.get("message", "") for res in want for r in res]
    assert sum("failed at path" in m for m in msgs) > 100 and sum(m.startswith("validation failure: ") for m in msgs) > 100
    assert sum("properties" in r for res in want for r in res) > 100
    # without resources: no messages, as kpe_report_results gives
    plain = engine.report_rows(ps, corpus, rows[:40])
    raw = engine.cv_masks(ps, corpus, raw=True)
    assert plain == [K.report_results(ps, v[int(i)], cv_mask_row=raw[int(i)]) for i in rows[:40]]


@pytest.mark.parametrize("keep", ["matrix", "fingerprints"])
def test_resident_scanner_reports_the_changed_rows(engine, keep):
    pols = large_policies() + [restricted_latest()]
    edited = json.loads(json.dumps(pols))
    target = cond_message_policy_set()[0]["metadata"]["name"]
    for p in edited:  # the policy's text changes under the same name: its messages may differ
        if p["metadata"]["name"] == target:
            for r in p["spec"]["rules"]:
                if "message" in r.get("validate", {}):
                    r["validate"]["message"] = "edited: " + r["validate"]["message"]
    edited = [p for p in edited if p["metadata"]["name"] != "restrict-sysctls"]  # and one policy leaves
    psa, psb = K.PolicySet(pols), K.PolicySet(edited)
    nd = K.synth_resources(0x77, 1200, mix=2)
    lines = [l for l in nd.split(b"\n") if l]
    plain = K.ResidentScanner(engine, nd, keep=keep)
    scanner = K.ResidentScanner(engine, nd, keep=keep, reports=True)
    with pytest.raises(K.KpeError):
        plain.reports([0])
    with pytest.raises(K.KpeError):
        scanner.reports([0])  # no apply yet
    first = scanner.apply(psa)
    assert sorted(first) == sorted(plain.apply(psa)) and scanner.last_stats == plain.last_stats
    changed = scanner.apply(psb, edited=[target])
    want = plain.apply(psb, edited=[target])
    assert sorted(changed) == sorted(want) and all(np.array_equal(changed[i], want[i]) for i in want)
    assert scanner.last_stats == plain.last_stats and set(scanner.last_stats) == {"rows", "changed"}
    assert 0 < len(changed) <= 1200
    rows = sorted(changed)
    got = scanner.reports(rows)
    v, _, _ = engine.fetch(psb, scanner.corpus)
    ref = per_row_reports(engine, psb, scanner.corpus, v, lines, rows)
    assert sorted(got) == rows
    for k, i in enumerate(rows):
        assert got[i] == ref[k], i
    assert any("edited: " in r.get("message", "") for i in rows for r in got[i])


def test_pattern_traces_of_a_mixed_cell_list(engine):
    """kpe_pattern_traces over foreach and plain cells in one list equals each cell asked alone."""
    ps = K.PolicySet(large_policies())
    corpus = K.Corpus(K.synth_resources(0x91, 700, mix=2))
    v, _, _ = engine.evaluate(ps, corpus)
    R = ps.num_rules
    _, _, psel = K.report_detail_need(ps)
    fe = np.array(["femsg" in n or "foreach" in n for n in ps.rule_names])
    needed = np.flatnonzero((((psel[None, :].astype(np.uint32) >> v) & 1) != 0).reshape(-1))
    rng = np.random.default_rng(3)
    cells = np.concatenate([rng.choice(needed, size=min(needed.size, 220), replace=False),
                            rng.integers(0, 700 * R, size=40)]).astype(np.uint64)
    rng.shuffle(cells)
    assert fe[(cells % R).astype(np.int64)].any() and (~fe[(cells % R).astype(np.int64)]).any()
    got = engine.pattern_traces(ps, corpus, cells)
    one = np.stack([engine.pattern_traces(ps, corpus, cells[k:k + 1])[0] for k in range(cells.size)])
    assert np.array_equal(got, one)
    assert (got[:, 0, 0] & 0x1000000).any()  # some record is valid
