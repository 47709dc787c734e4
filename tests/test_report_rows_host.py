"""Reports for a row list, host half (no GPU): the entry points are exported; kpe_report_detail_need
is tight in kind on the message policy sets; the host twin of the selection (kpe_report_cells_host)
equals a numpy restatement at every cap; the bulk renderer (kpe_report_results_rows) over the twin's
sparse lists is byte-identical to kpe_report_results_ex row by row, with 1 and with 16 threads, for
rows without a resource, a duplicate row and truncated lists; and the bodies of the two new kernels
(kyverno_amd/csrc/report_rows.inl) run lane by lane on the host under ASan / UBSan
(scripts/report_rows_check.cpp) give the double loop's lists."""
import ctypes
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import kyverno_amd as K
from kyverno_amd._lib import load
from kyverno_amd.engine import CTRACE_WORDS, RR_COND, RR_MASKS, RR_PATTERNS, TRACE_ROOTS, TRACE_WORDS, ReportRows
from tests.conftest import build_host_tool
from tests.policies import cond_message_policy_set, foreach_message_policy_set, restricted_latest, selector_policy

KPE_E_INVALID, KPE_E_STATE = 1, 5
PASS, FAIL, ERROR, SKIP = 1, 2, 4, 5
REC = TRACE_ROOTS * TRACE_WORDS
SENT = 0xA5
ALL = RR_MASKS | RR_COND | RR_PATTERNS


def chart_pattern_policies():
    from tests.test_gpu_pattern import chart_pattern_policies as f

    return f()


def test_symbols_exported():
    L = load()
    for name in ("kpe_report_detail_need", "kpe_fetch_report_rows", "kpe_report_cells_host", "kpe_report_results_rows"):
        assert hasattr(L, name), name
    for name in ("report_detail_need", "report_cells", "render_report_rows"):
        assert callable(getattr(K, name)), name
    for name in ("fetch_report_rows", "report_rows"):
        assert callable(getattr(K.Engine, name)), name
    assert callable(K.ResidentScanner.reports)


# ---- kpe_report_detail_need -------------------------------------------------------------------
def test_detail_need_of_a_podsecurity_program():
    m, c, p = K.report_detail_need(K.PolicySet([restricted_latest()]))
    assert m.tolist() == [K.SEL(FAIL)] * 3
    assert c.tolist() == [0] * 3 and p.tolist() == [0] * 3


@pytest.mark.parametrize("which", ["cond", "foreach", "chart"])
def test_detail_need_is_tight_in_kind(which):
    pols = {"cond": cond_message_policy_set, "foreach": foreach_message_policy_set, "chart": chart_pattern_policies}[which]()
    ps = K.PolicySet(pols)
    m, c, p = K.report_detail_need(ps)
    assert m.shape == c.shape == p.shape == (ps.num_rules,)
    never = K.SEL(0) | K.SEL(7) | K.SEL(6)  # NA, UNDECIDED (and the code no cell carries)
    assert not ((m | c | p) & never).any()
    assert not m[~np.array(ps.is_pss)].any()
    rules = {}  # "<policy>/<rule without the autogen prefix>" -> the rule's validate block
    for pol in pols:
        for r in pol["spec"]["rules"]:
            rules[(pol["metadata"]["name"], r["name"])] = r
    some = {"cond": 0, "pattern": 0}
    for j, full in enumerate(ps.rule_names):
        pname, rname = full.split("/", 1)
        r = rules[(pname, rname.replace("autogen-cronjob-", "").replace("autogen-", ""))]
        val = r.get("validate", {})
        walks = "pattern" in val or "anyPattern" in val or "pattern" in json.dumps(val.get("foreach", "")) \
            or "anyPattern" in json.dumps(val.get("foreach", ""))
        if not walks:
            assert p[j] == 0, full  # no pattern walk
        if "preconditions" not in r and "deny" not in val and "foreach" not in val:
            assert c[j] == 0, full  # nothing that could own a trace slot
        if "pattern" in val:
            assert p[j] & K.SEL(FAIL), full
        if isinstance(val.get("anyPattern"), list):  # one that is not a list always errors: no walk to read
            assert p[j] & K.SEL(FAIL) and p[j] & K.SEL(PASS), full
        some["cond"] += bool(c[j])
        some["pattern"] += bool(p[j])
    if which in ("cond", "foreach"):
        assert some["cond"] > 0
    if which in ("chart", "foreach"):
        assert some["pattern"] > 0


# ---- kpe_report_cells_host against numpy ------------------------------------------------------
_PROGRAMS = {}


def program_with_rules(R):
    """A real program of exactly R rules with need tables of every kind: message policies while
    they fit, then one-rule podSecurity selector policies (selectors disable autogen)."""
    if R in _PROGRAMS:
        return _PROGRAMS[R]
    pols = []
    left = R
    pool = [] if R == 1 else foreach_message_policy_set()[:2] + cond_message_policy_set()[:1] + [restricted_latest()]
    for pol in pool:
        n = K.PolicySet([pol]).num_rules
        if n <= left - (1 if R > 3 else 0):  # keep room for one selector policy
            pols.append(pol)
            left -= n
    pols += [selector_policy(f"sel{i}", selector={"matchLabels": {"app": f"a{i}"}}) for i in range(left)]
    ps = K.PolicySet(pols)
    assert ps.num_rules == R, (R, ps.num_rules)
    _PROGRAMS[R] = ps
    return ps


def random_inputs(seed, k, R):
    rng = np.random.default_rng(seed)
    v = rng.choice(np.arange(8, dtype=np.uint8), size=(k, R), p=[.4, .1, .2, .02, .1, .1, .03, .05])
    m = rng.integers(0, 1 << 32, size=(k, R), dtype=np.uint64).astype(np.uint32)
    cx = rng.integers(0, 1 << 32, size=(k, R, CTRACE_WORDS), dtype=np.uint64).astype(np.uint32)
    return v, m, cx


def spec_cells(ps, v, flags):
    """The three lists of compact cells, stated in numpy: cell k * R + r is listed for a kind iff
    (sel[r] >> v[k, r]) & 1 and the kind's flag is set."""
    out = []
    for bit, sel in zip((RR_MASKS, RR_COND, RR_PATTERNS), K.report_detail_need(ps)):
        hit = ((sel[None, :].astype(np.uint32) >> np.minimum(v, 31)) & 1).astype(bool) & (v < 8)
        out.append(np.flatnonzero(hit.reshape(-1)).astype(np.uint64) if flags & bit else np.zeros(0, np.uint64))
    return out


def guarded(n, dtype, words=1):
    """n * words elements and a sentinel tail: nothing past what a call may write changes."""
    a = np.full((n + 3) * words, SENT, dtype=np.uint8).repeat(np.dtype(dtype).itemsize).view(dtype)
    return a


def call_cells_host(ps, v, m, cx, flags, caps):
    cm, cc, cp = caps
    a = {"mc": guarded(cm, np.uint64), "mw": guarded(cm, np.uint32), "cc": guarded(cc, np.uint64),
         "cw": guarded(cc, np.uint32, CTRACE_WORDS), "pc": guarded(cp, np.uint64)}
    io = ReportRows(None, a["mc"].ctypes.data if cm else None, a["mw"].ctypes.data if cm else None, cm,
                    a["cc"].ctypes.data if cc else None, a["cw"].ctypes.data if cc else None, cc,
                    a["pc"].ctypes.data if cp else None, None, cp, 77, 77, 77)
    st = load().kpe_report_cells_host(ps.h, v.shape[0], v.ctypes.data if v.size else None,
                                      m.ctypes.data if v.size else None, cx.ctypes.data if v.size else None, flags,
                                      ctypes.byref(io))
    assert st == 0, load().kpe_last_error()
    return a, (io.mask_total, io.cond_total, io.pattern_total)


def check_lists(a, totals, caps, want, m, cx, what):
    """a: the guarded arrays of a call, want: the expected full lists; entries below min(total, cap)
    equal the expectation, every element past them is still the sentinel."""
    sent = {np.dtype(np.uint64): np.uint64(0xA5A5A5A5A5A5A5A5), np.dtype(np.uint32): np.uint32(0xA5A5A5A5)}
    assert tuple(totals) == tuple(len(w) for w in want), what
    for kind, (cells_key, words_key, nw) in enumerate((("mc", "mw", 1), ("cc", "cw", CTRACE_WORDS), ("pc", None, 0))):
        k = min(len(want[kind]), caps[kind])
        got = a[cells_key]
        assert np.array_equal(got[:k], want[kind][:k]), (what, kind)
        assert (got[k:] == sent[got.dtype]).all(), (what, kind, "cells past min(total, cap) written")
        if words_key:
            w = a[words_key]
            src = m.reshape(-1) if kind == 0 else cx.reshape(-1, CTRACE_WORDS)
            assert np.array_equal(w[:k * nw], src[want[kind][:k].astype(np.int64)].reshape(-1)), (what, kind)
            assert (w[k * nw:] == sent[w.dtype]).all(), (what, kind, "words past min(total, cap) written")


def row_counts(R):
    return sorted({0, 1, 255, 256, 257, 4097 // R, -(-4097 // R)})


@pytest.mark.parametrize("R", [1, 3, 5, 16, 17])
def test_cells_host_matches_numpy_at_every_cap(R):
    ps = program_with_rules(R)
    need = K.report_detail_need(ps)
    assert any(t.any() for t in need)
    for k in row_counts(R):
        v, m, cx = random_inputs(R * 1000 + k, k, R)
        for flags in (ALL, RR_MASKS, RR_COND | RR_PATTERNS, 0):
            want = spec_cells(ps, v, flags)
            tot = [len(w) for w in want]
            cap_sets = [(0, 0, 0), tuple(tot), tuple(max(t - 1, 0) for t in tot)] if flags == ALL else [tuple(tot)]
            for caps in cap_sets:
                a, totals = call_cells_host(ps, v, m, cx, flags, caps)
                check_lists(a, totals, caps, want, m, cx, (R, k, flags, caps))
    # the Python wrapper: a count call, then an exact call
    v, m, cx = random_inputs(R, 257, R)
    sp = K.report_cells(ps, v, m, cx)
    want = spec_cells(ps, v, ALL)
    assert np.array_equal(sp["mask_cells"], want[0]) and np.array_equal(sp["cond_cells"], want[1])
    assert np.array_equal(sp["pattern_cells"], want[2]) and sp["pattern_traces"].shape[0] == 0
    assert np.array_equal(sp["mask_words"], m.reshape(-1)[want[0].astype(np.int64)])
    assert np.array_equal(sp["cond_words"], cx.reshape(-1, CTRACE_WORDS)[want[1].astype(np.int64)])


def test_argument_checks_come_before_any_device_call():
    L = load()
    ps = program_with_rules(3)
    v, m, cx = random_inputs(1, 4, 3)
    io = ReportRows()
    # host twin
    assert L.kpe_report_cells_host(None, 4, v.ctypes.data, m.ctypes.data, cx.ctypes.data, ALL, ctypes.byref(io)) == KPE_E_INVALID
    assert L.kpe_report_cells_host(ps.h, 4, v.ctypes.data, m.ctypes.data, cx.ctypes.data, 8, ctypes.byref(io)) == KPE_E_INVALID
    assert L.kpe_report_cells_host(ps.h, 4, v.ctypes.data, m.ctypes.data, cx.ctypes.data, ALL, None) == KPE_E_INVALID
    io.mask_cap = 5  # a cap without its arrays
    assert L.kpe_report_cells_host(ps.h, 4, v.ctypes.data, m.ctypes.data, cx.ctypes.data, ALL, ctypes.byref(io)) == KPE_E_INVALID
    # device call: the same checks and the row bound need no device (a null device is refused first)
    io = ReportRows()
    rows = np.array([0, 1], dtype=np.uint64)
    corpus = K.Corpus(K.synth_resources(1, 2, mix=2))
    assert L.kpe_fetch_report_rows(None, ps.h, corpus.h, rows.ctypes.data, 2, ALL, ctypes.byref(io)) == KPE_E_INVALID
    # the renderer
    offs = np.zeros(5, dtype=np.uint64)
    assert L.kpe_report_results_rows(None, None, 4, ctypes.byref(io), None, None, None, 0, offs.ctypes.data) == -KPE_E_INVALID
    assert L.kpe_report_results_rows(ps.h, None, 4, None, None, None, None, 0, offs.ctypes.data) == -KPE_E_INVALID
    assert L.kpe_report_results_rows(ps.h, None, 4, ctypes.byref(io), None, None, None, 0, None) == -KPE_E_INVALID
    assert L.kpe_report_results_rows(ps.h, None, 4, ctypes.byref(io), None, None, None, 0, offs.ctypes.data) == -KPE_E_INVALID


# ---- the bulk renderer against the per-row renderer -------------------------------------------
@pytest.fixture(scope="module")
def condvm_bin():
    return build_host_tool("condvm_check")


@pytest.fixture(scope="module")
def render_case(condvm_bin, oracle, tmp_path_factory):
    """Policies of every kind over 1,500 synthetic rows: verdicts from the oracle, mask words random
    on the FAIL podSecurity cells (bit 31 on some), condition traces from the host-built condition
    VM on the two message sets' columns (zeros elsewhere), a synthetic record on every pattern cell."""
    from tests.test_foreach_messages import _host_vm_traces

    sets = [chart_pattern_policies(), cond_message_policy_set(), foreach_message_policy_set(), [restricted_latest()]]
    pols = [p for s in sets for p in s]
    ps = K.PolicySet(pols)
    R = ps.num_rules
    lines = [l for l in K.synth_resources(0x44, 1500, mix=2).split(b"\n") if l]
    nd = b"\n".join(lines)
    v = np.ascontiguousarray(oracle.validate(pols, nd, nthreads=8), dtype=np.uint8)
    N = v.shape[0]
    rng = np.random.default_rng(7)
    ncv = load().kpe_pss_num_cv()
    pss = np.array(ps.is_pss)
    m = np.zeros((N, R), dtype=np.uint32)
    hit = (v == FAIL) & pss[None, :]
    m[hit] = (rng.integers(1, 1 << ncv, size=int(hit.sum()), dtype=np.uint64)
              | (rng.integers(0, 2, size=int(hit.sum()), dtype=np.uint64) << np.uint64(31))).astype(np.uint32)
    cx = np.zeros((N, R, CTRACE_WORDS), dtype=np.uint32)
    col = {n: j for j, n in enumerate(ps.rule_names)}
    for sub in sets[1:3]:
        sps = K.PolicySet(sub)
        cols = [col[n] for n in sps.rule_names]
        _, scx = _host_vm_traces(condvm_bin, sub, lines, v[:, cols], tmp_path_factory.mktemp("vm"))
        cx[:, cols, :] = scx
    sp = K.report_cells(ps, v, m, cx)
    assert sp["mask_total"] > 100 and sp["cond_total"] > 1000 and sp["pattern_total"] > 100
    assert (sp["mask_words"] >> 31).any()
    cells = sp["pattern_cells"].astype(np.int64)
    rec = np.zeros((cells.size, TRACE_ROOTS, TRACE_WORDS), dtype=np.uint32)
    rec[:, :, 0] = 1 | (FAIL << 16) | 0x1000000  # one component, the root failed, KPE_TR_VALID
    rec[:, :, 1] = (0x80000000 | (cells % 7))[:, None].astype(np.uint32)  # KPE_TC_IDX
    sp["pattern_traces"] = rec
    dense = np.zeros((N * R, TRACE_ROOTS, TRACE_WORDS), dtype=np.uint32)
    dense[cells] = rec
    return {"ps": ps, "lines": lines, "corpus": K.Corpus(nd), "v": v, "m": m, "cx": cx, "sp": sp,
            "traces": dense.reshape(N, R, TRACE_ROOTS, TRACE_WORDS)}


def per_row(case, i, resource=True, masks=True, cond=True, traces=True):
    """kpe_report_results_ex over the row's dense inputs, as bytes."""
    ps, R = case["ps"], case["ps"].num_rules
    v = np.ascontiguousarray(case["v"][i])
    m = np.ascontiguousarray(case["m"][i]) if masks else None
    cx = np.ascontiguousarray(case["cx"][i]) if cond else None
    t = np.ascontiguousarray(case["traces"][i]) if traces else None
    raw = case["lines"][i] if resource else None
    a = K.engine.ReportArgs(ps.h, case["corpus"].h, v.ctypes.data, None if m is None else m.ctypes.data,
                            None if t is None else t.ctypes.data, None, raw, len(raw) if raw else 0,
                            None if cx is None else cx.ctypes.data)
    cap = 1 << 16
    buf = ctypes.create_string_buffer(cap)
    n = load().kpe_report_results_ex(ctypes.byref(a), buf, cap)
    assert 0 <= n < cap
    return buf.raw[:n]


def test_bulk_render_equals_the_per_row_renderer(render_case, monkeypatch):
    case = render_case
    N = case["v"].shape[0]
    want = [per_row(case, i) for i in range(N)]
    assert sum(b'"message"' in w for w in want) > 500
    outs = {}
    for threads in ("1", "16"):
        monkeypatch.setenv("KPE_REPORT_THREADS", threads)
        outs[threads] = K.render_report_rows(case["ps"], case["sp"], resources=case["lines"], corpus=case["corpus"], raw=True)
        bad = [i for i in range(N) if outs[threads][i] != want[i]]
        assert not bad, (threads, bad[:5], outs[threads][bad[0]], want[bad[0]])
    assert outs["1"] == outs["16"]
    parsed = K.render_report_rows(case["ps"], case["sp"], resources=case["lines"], corpus=case["corpus"])
    assert parsed[3] == json.loads(want[3])


def test_bulk_render_rows_without_a_resource_and_a_duplicate_row(render_case):
    case = render_case
    ps, R = case["ps"], case["ps"].num_rules
    busy = [int(i) for i in np.flatnonzero((case["v"] != 0).sum(axis=1) > 2)[:40]]
    rows = busy[:20] + [busy[3]] + busy[20:]  # a duplicate, out of order
    v, m, cx = case["v"][rows], case["m"][rows], case["cx"][rows]
    sp = K.report_cells(ps, v, m, cx)
    tr = case["traces"][rows].reshape(len(rows) * R, TRACE_ROOTS, TRACE_WORDS)
    sp["pattern_traces"] = tr[sp["pattern_cells"].astype(np.int64)]
    res = [None if k % 3 == 0 else case["lines"][i] for k, i in enumerate(rows)]
    got = K.render_report_rows(ps, sp, resources=res, corpus=case["corpus"], raw=True)
    for k, i in enumerate(rows):
        assert got[k] == per_row(case, i, resource=res[k] is not None), (k, i)
    assert got[20] == got[3] or res[20] is None or res[3] is None
    none = K.render_report_rows(ps, sp, resources=None, corpus=case["corpus"], raw=True)
    assert none == [per_row(case, i, resource=False) for i in rows]


@pytest.mark.parametrize("kind", ["mask", "cond", "pattern"])
def test_bulk_render_of_a_truncated_list(render_case, kind):
    """A list cut in the middle: the rows before the cut render as with the full list, the rows past
    it as the per-row call without that input."""
    case = render_case
    ps, R = case["ps"], case["ps"].num_rules
    N = case["v"].shape[0]
    sp = dict(case["sp"])
    cells_key, pay_key = {"mask": ("mask_cells", "mask_words"), "cond": ("cond_cells", "cond_words"),
                          "pattern": ("pattern_cells", "pattern_traces")}[kind]
    cut = sp[cells_key].size // 2
    cut_row = int(sp[cells_key][cut] // R)
    sp[cells_key], sp[pay_key] = sp[cells_key][:cut], sp[pay_key][:cut]
    got = K.render_report_rows(ps, sp, resources=case["lines"], corpus=case["corpus"], raw=True)
    changed = 0
    for i in range(N):
        if i == cut_row:
            continue
        full = per_row(case, i)
        if i < cut_row:
            assert got[i] == full, i
        else:
            want = per_row(case, i, masks=kind != "mask", cond=kind != "cond", traces=kind != "pattern")
            assert got[i] == want, i
            changed += want != full
    assert changed > 10  # the detail mattered for the rows past the cut


def test_bulk_render_small_buffer_returns_the_length(render_case):
    case = render_case
    ps, R = case["ps"], case["ps"].num_rules
    v = np.ascontiguousarray(case["v"][:5])
    io = ReportRows(v.ctypes.data, None, None, 0, None, None, 0, None, None, 0, 0, 0, 0)
    offs = np.full(7, 0xEE, dtype=np.uint64)
    n = load().kpe_report_results_rows(ps.h, None, 5, ctypes.byref(io), None, None, None, 0, offs.ctypes.data)
    want = [per_row(case, i, resource=False, masks=False, cond=False, traces=False) for i in range(5)]
    assert n == sum(len(w) for w in want)
    assert offs[:6].tolist() == np.cumsum([0] + [len(w) for w in want]).tolist() and offs[6] == 0xEE
    buf = ctypes.create_string_buffer(n + 1)
    assert load().kpe_report_results_rows(ps.h, None, 5, ctypes.byref(io), None, None, buf, n + 1, offs.ctypes.data) == n
    assert buf.raw[:n] == b"".join(want)


# ---- the kernels' bodies under ASan / UBSan ---------------------------------------------------
@pytest.fixture(scope="module")
def rr_check():
    return build_host_tool("report_rows_check")


# (R, N, rows, grid): rows name first / last row, duplicates, descending runs; nrows * R is no
# multiple of the 4096-cell tile
def _row_list(seed, N, k):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, N, size=k, dtype=np.uint64)
    if k >= 4:
        rows[0], rows[1], rows[2], rows[3] = 0, N - 1, N - 1, 0
    if k >= 40:
        rows[10:40] = np.sort(rows[10:40])[::-1]
    return rows


HARNESS = [(1, 70, 5000, 3), (3, 300, 2000, 2), (5, 257, 1000, 7), (16, 100, 300, 1), (17, 90, 500, 4),
           (204, 64, 41, 3), (16385, 3, 2, 2), (3, 5, 0, 1), (3, 5, 1, 1)]


@pytest.mark.parametrize("R,N,k,grid", HARNESS, ids=[f"r{c[0]}-n{c[1]}-k{c[2]}" for c in HARNESS])
def test_kernel_bodies_under_asan_match_the_double_loop(rr_check, tmp_path, R, N, k, grid):
    rng = np.random.default_rng(R * 7 + k)
    nmsg = 0
    slot = np.zeros(R, dtype=np.uint32)
    need = np.zeros((3, R), dtype=np.uint8)
    for r in range(R):  # random tables, tight in kind: bit 0 clear; cond only with a slot
        kind = rng.integers(0, 5)
        if kind == 0:
            need[0, r] = K.SEL(FAIL)
        elif kind in (1, 2):
            w = 1 if kind == 1 else 4
            slot[r] = (nmsg << 3) | w
            nmsg += w
            need[1, r] = int(rng.integers(0, 128)) * 2 & 0x7E
            if kind == 2:
                need[2, r] = K.SEL(FAIL) | K.SEL(ERROR)
        elif kind == 3:
            need[2, r] = K.SEL(FAIL) | (K.SEL(PASS) if rng.integers(0, 2) else 0)
    v = rng.choice(np.arange(8, dtype=np.uint8), size=(N, R), p=[.55, .1, .15, .02, .08, .05, .02, .03])
    masks = rng.integers(0, 1 << 32, size=(N, R), dtype=np.uint64).astype(np.uint32)
    mtrace = rng.integers(0, 1 << 32, size=(N, max(nmsg, 1)), dtype=np.uint64).astype(np.uint32)[:, :nmsg]
    rows = _row_list(k, N, k) if k else np.zeros(0, dtype=np.uint64)
    # the double loop
    cv = v[rows.astype(np.int64)] if k else np.zeros((0, R), dtype=np.uint8)
    hits = [np.flatnonzero((((need[t][None, :].astype(np.uint32) >> cv) & 1).astype(bool)).reshape(-1)) for t in range(3)]
    tot = [len(h) for h in hits]
    cap_sets = [tuple(tot), (0, 0, 0), tuple(t // 2 for t in tot), (min(tot[0], 3), max(tot[1] - 1, 0), min(tot[2], 70))]
    for caps in cap_sets:
        case = tmp_path / "case.bin"
        with open(case, "wb") as f:
            f.write(struct.pack("<QQIIIIQQQ", N, k, R, grid, nmsg, 0, *caps))
            f.write(need.tobytes() + slot.tobytes() + rows.tobytes() + v.tobytes() + masks.tobytes()
                    + np.ascontiguousarray(mtrace).tobytes())
        outp = tmp_path / "out.bin"
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
        res = subprocess.run([rr_check, str(case), str(outp)], env=env, capture_output=True, text=True)
        assert res.returncode == 0, (caps, res.stdout, res.stderr)
        raw = outp.read_bytes()
        got_tot = struct.unpack_from("<QQQ", raw, 0)
        assert list(got_tot) == tot, caps
        off = 24
        km, kc, kp = (min(t, c) for t, c in zip(tot, caps))
        mc = np.frombuffer(raw, np.uint64, km, off); off += km * 8
        mw = np.frombuffer(raw, np.uint32, km, off); off += km * 4
        cc = np.frombuffer(raw, np.uint64, kc, off); off += kc * 8
        cw = np.frombuffer(raw, np.uint32, kc * 4, off).reshape(kc, 4); off += kc * 16
        pc = np.frombuffer(raw, np.uint64, kp, off); off += kp * 8
        pa = np.frombuffer(raw, np.uint64, kp, off); off += kp * 8
        assert off == len(raw)
        assert np.array_equal(mc, hits[0][:km]) and np.array_equal(cc, hits[1][:kc]) and np.array_equal(pc, hits[2][:kp])
        ri = rows.astype(np.int64)
        assert np.array_equal(mw, masks[ri[mc.astype(np.int64) // R], mc.astype(np.int64) % R])
        assert np.array_equal(pa.astype(np.int64), ri[pc.astype(np.int64) // R] * R + pc.astype(np.int64) % R)
        want_cw = np.zeros((kc, 4), dtype=np.uint32)
        for j, cell in enumerate(cc.astype(np.int64)):
            e = int(slot[cell % R])
            want_cw[j, :e & 7] = mtrace[ri[cell // R], (e >> 3):(e >> 3) + (e & 7)]
        assert np.array_equal(cw, want_cw)
