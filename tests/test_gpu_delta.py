"""Result deltas on the device: kpe_results_keep, kpe_changed_rows and kpe_delta_transitions against
their host twins over the two matrices kpe_fetch returns. Exact integer comparisons: the matrices
themselves are pinned to the oracle by the parity suites; these tests pin the comparison to the
matrices.

Each case evaluates program A, keeps its result, evaluates program B on the same uploaded corpus and
asks for the rows that changed. Shapes: the smallest at which each mechanism can go wrong. A block
of the flag pass takes groups of clamp(4096 / max(Rn, Ro), 1, 1024) whole rows on at most 2048
blocks and stages the kept rows in LDS from the group's first byte rounded down to 16; with
Rn != Ro the two sides have different skews. 682 / 683 is the group edge for R = 6; 45000 rows of
204 rules are 2250 groups, more than the grid; the row list is compacted 4096 flags per tile."""
import copy
import functools

import numpy as np
import pytest

import kyverno_amd as K
from kyverno_amd._lib import load
from tests.policies import c3_policy_set, parity_policy_set, pss_policy, restricted_latest, selector_policy

pytestmark = pytest.mark.gpu

FAIL, ERROR, SKIP = 2, 4, 5
KPE_E_STATE = 5


@functools.lru_cache(maxsize=None)
def pair(cfg):
    """(PolicySet A, PolicySet B, synth seed, synth mix, (Ro, Rn)) of a policy edit."""
    if cfg == "r1-r1":  # selectors disable autogen: one rule; the level changes
        mk = lambda level: [selector_policy("wild-both", level=level, selector={"matchLabels": {"*": "*"}})]
        return K.PolicySet(mk("baseline")), K.PolicySet(mk("restricted")), 0xC4, K.SYNTH_SELECTORS, (1, 1)
    if cfg == "r3-r3":
        b = restricted_latest()
        b["spec"]["rules"][0]["validate"]["podSecurity"]["level"] = "baseline"
        return K.PolicySet([restricted_latest()]), K.PolicySet([b]), 0xC2, K.SYNTH_MIXED, (3, 3)
    if cfg in ("r3-r6", "r6-r3"):  # a policy added in front (the map shifts) or removed (columns disappear)
        a = [restricted_latest()]
        b = [pss_policy("added", "baseline", extra_match={"namespaces": ["ns-00*"]})] + a
        if cfg == "r6-r3":
            a, b = b, a
        return K.PolicySet(a), K.PolicySet(b), 0xC2, K.SYNTH_MIXED, ((3, 6) if cfg == "r3-r6" else (6, 3))
    if cfg == "r18-r15":  # reordered, one policy gone, one edited
        P = copy.deepcopy(parity_policy_set())
        a = [restricted_latest()] + P[1:6]
        P[4]["spec"]["rules"][0]["validate"]["podSecurity"]["version"] = "v1.0"
        b = [P[5], restricted_latest(), P[1], P[3], P[4]]
        return K.PolicySet(a), K.PolicySet(b), 21, K.SYNTH_MIXED, (18, 15)
    if cfg == "r204-r204":
        b = c3_policy_set()
        for i in (7, 90, 150):
            for rule in b[i]["spec"]["rules"]:
                rule["exclude"] = {"any": [{"resources": {"namespaces": ["team-1*"]}}]}
        return K.PolicySet(c3_policy_set()), K.PolicySet(b), 0xC3, K.SYNTH_C3, (204, 204)
    raise KeyError(cfg)


@pytest.fixture(scope="module")
def engine():
    return K.Engine(ordinal=0)


def edited(engine, cfg, n):
    """A evaluated and kept, B evaluated: (A, B, corpus, A's matrix, B's matrix, the map by name)."""
    psa, psb, seed, mix, (Ro, Rn) = pair(cfg)
    assert (psa.num_rules, psb.num_rules) == (Ro, Rn)
    corpus = K.Corpus(K.synth_resources(seed, n, mix=mix)).upload(engine.device)
    assert corpus.n == n
    engine.evaluate_async(psa, corpus)
    va, _, _ = engine.fetch(psa, corpus)
    engine.keep_results(psa, corpus)
    engine.evaluate_async(psb, corpus)
    vb, _, _ = engine.fetch(psb, corpus)
    assert not (va == 7).any() and not (vb == 7).any()  # no undecided cell
    return psa, psb, corpus, va, vb, K.column_map(psa.rule_names, psb.rule_names)


def check_against_twin(engine, psb, corpus, va, vb, cmap, column_map=None, always=0):
    want_rows, want_vr, want_total = K.changed_rows(va, vb, cmap, always)
    rows, vr, total = engine.changed_rows(psb, corpus, column_map=column_map, always=always)
    print(f"changed rows: device {total}, twin {want_total} of {corpus.n}")
    assert total == want_total
    assert rows.dtype == np.uint64 and vr.dtype == np.uint8 and vr.shape == (want_total, psb.num_rules)
    assert np.array_equal(rows, want_rows), np.setxor1d(rows, want_rows)[:8].tolist()
    assert np.array_equal(vr, want_vr)
    return total


SHAPES = ([("r1-r1", n) for n in (1, 15, 16, 17, 1023, 1024, 1025, 4097)] +
          [("r3-r3", n) for n in (1, 5, 6, 64, 1365, 1366, 5000)] +
          [(c, n) for c in ("r3-r6", "r6-r3") for n in (64, 682, 683, 5000)] +
          [("r18-r15", n) for n in (227, 228, 4096)] +
          [("r204-r204", n) for n in (21, 2000, 20100, 45000)])

# changed rows of the edits at some shapes, from the oracle's matrices
KNOWN = {("r1-r1", 1025): 35, ("r1-r1", 4097): 126, ("r3-r3", 1366): 65, ("r3-r3", 5000): 264,
         ("r3-r6", 683): 57, ("r6-r3", 683): 57, ("r3-r6", 5000): 362, ("r6-r3", 5000): 362,
         ("r18-r15", 228): 166, ("r18-r15", 4096): 2962, ("r204-r204", 2000): 67, ("r204-r204", 20100): 712}


@pytest.mark.parametrize("cfg,n", SHAPES, ids=[f"{c}-{n}" for c, n in SHAPES])
def test_changed_rows_and_transitions_match_host(engine, cfg, n):
    psa, psb, corpus, va, vb, cmap = edited(engine, cfg, n)
    Ro, Rn = psa.num_rules, psb.num_rules
    assert engine.kept_rule_names(corpus) == psa.rule_names
    # the map by rule name, built by the library
    got_map = np.zeros(Rn, dtype=np.int32)
    assert load().kpe_delta_column_map(corpus.h, psb.h, got_map.ctypes.data) == 0
    assert np.array_equal(got_map, cmap)
    total = check_against_twin(engine, psb, corpus, va, vb, cmap)
    if n >= 683:
        assert 0 < total < n
    if (cfg, n) in KNOWN:
        assert total == KNOWN[(cfg, n)]
    # the same map passed explicitly; without the verdict rows
    check_against_twin(engine, psb, corpus, va, vb, cmap, column_map=cmap)
    rows, vr, t2 = engine.changed_rows(psb, corpus, with_verdicts=False)
    assert t2 == total and rows.size == total and vr.shape == (0, Rn)

    want = K.delta_transitions(va, vb, cmap)
    got = engine.delta_transitions(psb, corpus)
    assert got.shape == (Rn, 8, 8) and got.dtype == np.uint64
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()
    assert (got.reshape(Rn, 64).sum(axis=1) == n).all()


ALWAYS_SHAPES = [("r3-r3", 1366), ("r3-r6", 683), ("r6-r3", 683), ("r18-r15", 228), ("r204-r204", 2000)]


@pytest.mark.parametrize("cfg,n", ALWAYS_SHAPES, ids=[f"{c}-{n}" for c, n in ALWAYS_SHAPES])
def test_always_mask_adds_the_twins_rows(engine, cfg, n):
    psa, psb, corpus, va, vb, cmap = edited(engine, cfg, n)
    Rn = psb.num_rules
    base = check_against_twin(engine, psb, corpus, va, vb, cmap)
    always = np.where(np.arange(Rn) % 2 == 1, K.SEL(FAIL), 0).astype(np.uint8)
    total = check_against_twin(engine, psb, corpus, va, vb, cmap, always=always)
    assert (vb[:, 1::2] == FAIL).any() and base <= total <= n


@pytest.mark.parametrize("cfg,n", [("r3-r6", 683), ("r18-r15", 228)])
def test_map_of_no_partner_changes_every_row_with_a_response(engine, cfg, n):
    psa, psb, corpus, va, vb, _ = edited(engine, cfg, n)
    none = np.full(psb.num_rules, -1, dtype=np.int32)
    total = check_against_twin(engine, psb, corpus, va, vb, none, column_map=none)
    rows, _, _ = engine.changed_rows(psb, corpus, column_map=none)
    want = np.flatnonzero((va != 0).any(axis=1) | (vb != 0).any(axis=1)).astype(np.uint64)
    assert np.array_equal(rows, want) and total == want.size
    t = engine.delta_transitions(psb, corpus, column_map=none)
    assert np.array_equal(t, K.delta_transitions(va, vb, none)) and not t[:, 1:, :].any()


@pytest.mark.parametrize("cfg,n", [("r3-r3", 1366), ("r204-r204", 2000)])
def test_same_program_changes_nothing(engine, cfg, n):
    psa, _, seed, mix, _ = pair(cfg)
    corpus = K.Corpus(K.synth_resources(seed, n, mix=mix)).upload(engine.device)
    engine.evaluate_async(psa, corpus)
    engine.keep_results(psa, corpus)
    engine.evaluate_async(psa, corpus)
    v, _, _ = engine.fetch(psa, corpus)
    ident = np.arange(psa.num_rules, dtype=np.int32)
    for cmap in (None, ident):
        rows, vr, total = engine.changed_rows(psa, corpus, column_map=cmap)
        assert total == 0 and rows.size == 0 and vr.shape == (0, psa.num_rules)
    t = engine.delta_transitions(psa, corpus)
    assert np.array_equal(t, K.delta_transitions(v, v, ident))
    off = t.copy()
    off[:, np.arange(8), np.arange(8)] = 0
    assert not off.any() and (t.reshape(-1, 64).sum(axis=1) == n).all()


def test_cap_leaves_the_rest_untouched(engine):
    psa, psb, corpus, va, vb, cmap = edited(engine, "r18-r15", 4096)
    L = load()
    Rn = psb.num_rules
    want_rows, want_vr, total = K.changed_rows(va, vb, cmap)
    assert total > 100
    h = (engine.device.h, psb.h, corpus.h)
    assert L.kpe_changed_rows(*h, None, None, None, None, 0) == total  # count only
    cap = total // 2
    rows = np.full(total + 8, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    vr = np.full((total + 8, Rn), 0xA5, dtype=np.uint8)
    assert L.kpe_changed_rows(*h, cmap.ctypes.data, None, rows.ctypes.data, vr.ctypes.data, cap) == total
    assert np.array_equal(rows[:cap], want_rows[:cap]) and np.array_equal(vr[:cap], want_vr[:cap])
    assert (rows[cap:] == np.uint64(0xDEADBEEFDEADBEEF)).all() and (vr[cap:] == 0xA5).all()
    # a generous cap: everything, and only that, is written
    rows[:] = np.uint64(0xDEADBEEFDEADBEEF)
    assert L.kpe_changed_rows(*h, None, None, rows.ctypes.data, None, 1 << 40) == total
    assert np.array_equal(rows[:total], want_rows) and (rows[total:] == np.uint64(0xDEADBEEFDEADBEEF)).all()
    # the binding: cap through Engine.changed_rows
    r2, v2, t2 = engine.changed_rows(psb, corpus, cap=cap)
    assert t2 == total and np.array_equal(r2, want_rows[:cap]) and np.array_equal(v2, want_vr[:cap])
    # a map the kept result does not have
    bad = cmap.copy()
    bad[0] = psa.num_rules
    assert L.kpe_changed_rows(*h, bad.ctypes.data, None, None, None, 0) == -1  # KPE_E_INVALID


def test_queries_need_a_kept_result_and_an_evaluation(engine):
    psa, psb, seed, mix, _ = pair("r3-r6")
    corpus = K.Corpus(K.synth_resources(seed, 64, mix=mix)).upload(engine.device)
    queries = lambda ps: (lambda: engine.changed_rows(ps, corpus), lambda: engine.delta_transitions(ps, corpus))

    def refused(ps):
        for q in queries(ps):
            with pytest.raises(K.KpeError) as e:
                q()
            assert e.value.status == KPE_E_STATE

    with pytest.raises(K.KpeError) as e:
        engine.keep_results(psa, corpus)  # no evaluation yet
    assert e.value.status == KPE_E_STATE
    engine.evaluate_async(psa, corpus)
    refused(psa)  # nothing kept
    assert engine.kept_rule_names(corpus) is None
    engine.keep_results(psa, corpus)
    assert engine.changed_rows(psa, corpus)[2] == 0
    refused(psb)  # kept, but psb was not evaluated on this corpus
    engine.evaluate_async(psb, corpus)
    engine.changed_rows(psb, corpus)
    refused(psa)  # the corpus now holds psb's evaluation
    engine.drop_results(corpus)
    assert engine.kept_rule_names(corpus) is None
    refused(psb)
    # a re-upload drops a kept result too
    engine.keep_results(psb, corpus)
    assert engine.kept_rule_names(corpus) == psb.rule_names
    corpus.upload(engine.device)
    assert engine.kept_rule_names(corpus) is None


def test_kept_result_survives_another_programs_evaluation(engine):
    psa, psb, corpus, va, vb, cmap = edited(engine, "r3-r6", 683)
    third, _, _, _, _ = pair("r18-r15")
    engine.evaluate_async(third, corpus)  # rebinds the corpus: the binding's buffers are rebuilt
    vc, _, _ = engine.fetch(third, corpus)
    cmap_c = K.column_map(psa.rule_names, third.rule_names)
    check_against_twin(engine, third, corpus, va, vc, cmap_c)
    engine.evaluate_async(psb, corpus)
    assert check_against_twin(engine, psb, corpus, va, vb, cmap) == 57
    assert np.array_equal(engine.delta_transitions(psb, corpus), K.delta_transitions(va, vb, cmap))


def test_resident_scanner_returns_the_twins_rows(engine):
    psa, psb, seed, mix, _ = pair("r18-r15")
    nd = K.synth_resources(seed, 228, mix=mix)
    corpus = K.Corpus(nd)
    va, _, _ = engine.evaluate(psa, corpus)
    vb, _, _ = engine.evaluate(psb, corpus)
    sc = K.ResidentScanner(engine, nd)
    first = sc.apply(psa)
    assert sorted(first) == np.flatnonzero((va != 0).any(axis=1)).tolist()
    assert all(np.array_equal(first[i], va[i]) for i in first)
    cmap = K.column_map(psa.rule_names, psb.rule_names)
    edited_pols = {"pol-baseline-v1-22"}  # the policy whose version changed
    always = np.array([(K.SEL(FAIL) | K.SEL(ERROR) | K.SEL(SKIP)) if nm.split("/", 1)[0] in edited_pols else 0
                       for nm in psb.rule_names], dtype=np.uint8)
    assert always.any()
    want_rows, want_vr, total = K.changed_rows(va, vb, cmap, always)
    got = sc.apply(psb, edited=edited_pols)
    assert sorted(got) == want_rows.tolist() and sc.last_stats == {"rows": 228, "changed": total}
    assert all(np.array_equal(got[int(i)], want_vr[k]) for k, i in enumerate(want_rows))
    assert sc.apply(psb) == {}  # nothing changed since
