"""Policy edits on a kept result, on the device: kpe_results_splice and kpe_spliced_rows.

Each case is a policy edit A -> B expressed as the caller of ResidentScanner.apply_edit expresses it:
A evaluated and kept, `sub` the policies of B that differ from A's (edited or added) compiled alone,
`removed` the names that vanished. For every case
  (i)   the columns of sub evaluated alone equal B's columns of the same names from a full
        evaluation of B on the same corpus (the claim the whole feature rests on),
  (ii)  the spliced kept matrix, read back, equals B's full matrix byte for byte,
  (iii) the kept rule names are B's,
  (iv)  the changed rows and their verdict rows are exactly the twin's over the two full matrices
        (K.changed_rows, the specification of kpe_changed_rows), count-only and cap < total included,
  (v)   a plain changed_rows(B) after a full evaluation of B returns nothing.
Exact integer comparisons. Shapes: the smallest at which each mechanism can go wrong. A block of the
pass takes groups of clamp(4096 / max(Ro, Rs, rn), 1, 1024) whole rows on at most
kpe_splice_max_groups() blocks; the three sides of a group have different skews against 16 bytes
whenever their widths differ."""
import copy
import functools

import numpy as np
import pytest

import kyverno_amd as K
from kyverno_amd._lib import load
from tests.policies import (VAR_UNDECIDED_OK, c3_policy_set, cond_policy_set, parity_policy_set, pss_policy,
                            restricted_latest, selector_policy, var_policy_set)

pytestmark = pytest.mark.gpu

KPE_E_STATE = 5
NS_EXCLUDE = {"any": [{"resources": {"namespaces": ["team-1*", "ns-00*"]}}]}


def with_exclude(pol):
    pol = copy.deepcopy(pol)
    for rule in pol["spec"]["rules"]:
        rule["exclude"] = copy.deepcopy(NS_EXCLUDE)
    return pol


def mixed_set():
    """Condition rules, pattern-variable rules, an applyRules: One policy and a namespaceSelector."""
    vs = copy.deepcopy(var_policy_set())
    for p in vs:  # the rules the device documents as beyond its limits are not part of this claim
        p["spec"]["rules"] = [r for r in p["spec"]["rules"] if r["name"] not in VAR_UNDECIDED_OK]
    one = pss_policy("one", "baseline", "latest", apply_one=True)
    one["spec"]["rules"].append({"name": "second", "match": {"any": [{"resources": {"kinds": ["Pod"]}}]},
                                 "validate": {"podSecurity": {"level": "restricted", "version": "latest"}}})
    return (cond_policy_set() + vs + [one] +
            [selector_policy("ns-prod", kinds=("Pod",), ns_selector={"matchLabels": {"env": "prod"}})])


@functools.lru_cache(maxsize=None)
def pair(cfg):
    """(policies A, policies B, synth seed, synth mix, namespace labels or None, (Ro, Rs, rn))."""
    if cfg == "r1-r1":  # selectors disable autogen: one rule; the level changes
        mk = lambda level: [selector_policy("wild-both", level=level, selector={"matchLabels": {"*": "*"}})]
        return mk("baseline"), mk("restricted"), 0xC4, K.SYNTH_SELECTORS, None, (1, 1, 1)
    if cfg == "r3-r3":
        b = restricted_latest()
        b["spec"]["rules"][0]["validate"]["podSecurity"]["level"] = "baseline"
        return [restricted_latest()], [b], 0xC2, K.SYNTH_MIXED, None, (3, 3, 3)
    if cfg in ("r3-r6", "r6-r3"):  # a policy added (appended), or removed in front (columns disappear)
        a = [restricted_latest()]
        added = pss_policy("added", "baseline", extra_match={"namespaces": ["ns-00*"]})
        if cfg == "r3-r6":
            return a, a + [added], 0xC2, K.SYNTH_MIXED, None, (3, 3, 6)
        return [added] + a, a, 0xC2, K.SYNTH_MIXED, None, (6, 0, 3)
    if cfg == "r18-r15":  # one policy gone, one edited
        P = copy.deepcopy(parity_policy_set())
        a = [restricted_latest()] + P[1:6]
        b = copy.deepcopy(a)
        b[4]["spec"]["rules"][0]["validate"]["podSecurity"]["version"] = "v1.0"
        del b[2]
        return a, b, 21, K.SYNTH_MIXED, None, (18, 3, 15)
    if cfg in ("r204-r204", "r204-r205"):
        a = c3_policy_set()
        b = c3_policy_set()
        if cfg == "r204-r204":
            b[90] = with_exclude(b[90])
            return a, b, 0xC3, K.SYNTH_C3, None, (204, 1, 204)
        second = with_exclude(b[90])["spec"]["rules"][0]
        second["name"] += "-b"
        b[90]["spec"]["rules"].append(second)
        return a, b, 0xC3, K.SYNTH_C3, None, (204, 2, 205)
    if cfg in ("mixed-cond-sel", "mixed-var-one"):
        a = mixed_set()
        b = copy.deepcopy(a)
        for i in ((0, 3) if cfg == "mixed-cond-sel" else (1, 2)):
            b[i] = with_exclude(b[i])
        return a, b, 0xA3, K.SYNTH_MIXED, K.synth_ns_labels(0xA3, 10000, mix=3), None
    raise KeyError(cfg)


def edit_of(a, b):
    """(the policies of b that a does not hold as they are, the names of a's that b lacks)."""
    old = {p["metadata"]["name"]: p for p in a}
    new = {p["metadata"]["name"] for p in b}
    return [p for p in b if old.get(p["metadata"]["name"]) != p], [n for n in old if n not in new]


@pytest.fixture(scope="module")
def engine():
    return K.Engine(ordinal=0)


MAX_GROUPS = 2048  # kpe_splice_max_groups(); the library is not loaded while the tests are collected


def group_rows(cfg):
    """splice.inl splice_rows_per_group, restated (test_tiling_constants holds both to the library)."""
    return max(1, min(1024, 4096 // max(pair(cfg)[5] + (1,))))


def test_tiling_constants():
    for cfg in ("r1-r1", "r3-r3", "r3-r6", "r6-r3", "r18-r15", "r204-r204", "r204-r205"):
        assert load().kpe_splice_group_rows(*pair(cfg)[5]) == group_rows(cfg)
    assert load().kpe_splice_max_groups() == MAX_GROUPS


def shapes():
    out = [("r1-r1", n) for n in (1, 15, 16, 17)]
    for cfg in ("r3-r3", "r3-r6", "r6-r3"):
        g = group_rows(cfg)
        out += [(cfg, g - 1), (cfg, g), (cfg, g + 1)]
    out += [("r18-r15", 228), ("r18-r15", 4096)]
    # more groups than the grid: the persistent loop of every block runs twice
    many = (MAX_GROUPS + 2) * group_rows("r204-r204") + 7
    out += [("r204-r204", 21), ("r204-r204", many), ("r204-r205", 21), ("r204-r205", 2000)]
    out += [("mixed-cond-sel", 4096), ("mixed-var-one", 4096)]
    return out


SHAPES = shapes()


@pytest.mark.parametrize("cfg,n", SHAPES, ids=[f"{c}-{n}" for c, n in SHAPES])
def test_splice_equals_the_full_evaluation(engine, cfg, n):
    a, b, seed, mix, nsl, widths = pair(cfg)
    sub_pols, removed = edit_of(a, b)
    psa, psb, sub = K.PolicySet(a), K.PolicySet(b), K.PolicySet(sub_pols)
    Ro, Rs, rn = psa.num_rules, sub.num_rules, psb.num_rules
    if widths is not None:
        assert (Ro, Rs, rn) == widths
    else:
        assert Rs > 0 and rn == Ro
    corpus = K.Corpus(K.synth_resources(seed, n, mix=mix), nsl).upload(engine.device)
    assert corpus.n == n
    engine.evaluate_async(psb, corpus)
    vb, _, _ = engine.fetch(psb, corpus)
    engine.evaluate_async(psa, corpus)
    va, _, _ = engine.fetch(psa, corpus)
    engine.keep_results(psa, corpus)
    assert not (va == 7).any() and not (vb == 7).any()  # no undecided cell under the full compilation

    # the plan the library builds, against the twin
    plan, partner = K.splice_plan(psa.rule_names, sub.rule_names, removed)
    assert np.array_equal(engine.splice_plan(sub, corpus, removed), plan)
    assert K.splice_names(psa.rule_names, sub.rule_names, plan) == psb.rule_names

    always = np.array([K.MESSAGE_CODES if k % 2 == 0 else 0 for k in range(Rs)], dtype=np.uint8)
    if Rs:
        engine.evaluate_async(sub, corpus)
        e, _, _ = engine.fetch(sub, corpus)
        assert not (e == 7).any()  # nor under the partial one
        # (i) a policy compiled alone gives the columns it gives inside the full program
        cols = [psb.rule_names.index(nm) for nm in sub.rule_names]
        bad = np.argwhere(e != vb[:, cols])
        assert bad.size == 0, [(int(i), sub.rule_names[int(s)], int(e[i, s]), int(vb[i, cols[s]])) for i, s in bad[:5]]
    total = engine.splice_results(sub, corpus, removed, always)

    # (ii), (iii)
    kept = engine.kept_results(corpus)
    assert kept.shape == vb.shape and np.array_equal(kept, vb), np.argwhere(kept != vb)[:5].tolist()
    assert engine.kept_rule_names(corpus) == psb.rule_names

    # (iv) the twin over the two full matrices, `always` expanded to B's columns
    cmap = K.column_map(psa.rule_names, psb.rule_names)
    always_b = np.array([0 if p >= 0 else always[-1 - p] for p in plan], dtype=np.uint8)
    want_rows, want_vr, want_total = K.changed_rows(va, vb, cmap, always_b)
    print(f"{cfg} n={n}: changed rows device {total}, twin {want_total}")
    assert total == want_total
    rows, vr, t = engine.spliced_rows(corpus)
    assert t == total and rows.dtype == np.uint64 and vr.shape == (total, rn)
    assert np.array_equal(rows, want_rows), np.setxor1d(rows, want_rows)[:8].tolist()
    assert np.array_equal(vr, want_vr)
    if n >= 600:
        assert 0 < total < n
    # count only; without the verdict rows; cap < total leaves the rest alone (and may be asked again)
    assert load().kpe_spliced_rows(engine.device.h, corpus.h, None, None, 0) == total
    r2, v2, t2 = engine.spliced_rows(corpus, with_verdicts=False)
    assert t2 == total and np.array_equal(r2, rows) and v2.shape == (0, rn)
    if total >= 2:
        cap = total // 2
        rbuf = np.full(cap + 3, 0xAB, dtype=np.uint64)
        vbuf = np.full((cap + 3, rn), 0xCD, dtype=np.uint8)
        assert load().kpe_spliced_rows(engine.device.h, corpus.h, rbuf.ctypes.data, vbuf.ctypes.data, cap) == total
        assert np.array_equal(rbuf[:cap], rows[:cap]) and (rbuf[cap:] == 0xAB).all()
        assert np.array_equal(vbuf[:cap], vr[:cap]) and (vbuf[cap:] == 0xCD).all()

    # (v) the spliced result is a kept result like any other
    engine.evaluate_async(psb, corpus)
    rows, _, t = engine.changed_rows(psb, corpus)
    assert t == 0 and rows.size == 0


def test_splice_needs_a_kept_result_and_the_evaluation_of_sub(engine):
    a, b, seed, mix, _, _ = pair("r3-r3")
    psa, sub = K.PolicySet(a), K.PolicySet(b)
    corpus = K.Corpus(K.synth_resources(seed, 64, mix=mix)).upload(engine.device)
    engine.evaluate_async(sub, corpus)
    with pytest.raises(K.KpeError) as e:  # nothing kept
        engine.splice_results(sub, corpus)
    assert e.value.status == KPE_E_STATE
    engine.evaluate_async(psa, corpus)
    engine.keep_results(psa, corpus)
    with pytest.raises(K.KpeError) as e:  # the last evaluation is of A, not of sub
        engine.splice_results(sub, corpus)
    assert e.value.status == KPE_E_STATE
    with pytest.raises(K.KpeError) as e:  # no splice yet
        engine.spliced_rows(corpus)
    assert e.value.status == KPE_E_STATE
    engine.evaluate_async(sub, corpus)
    total = engine.splice_results(sub, corpus)
    assert engine.spliced_rows(corpus)[2] == total
    # a second splice with the same sub changes nothing and reuses the spare buffer
    engine.evaluate_async(sub, corpus)
    assert engine.splice_results(sub, corpus) == 0
    assert engine.spliced_rows(corpus)[0].size == 0
    engine.keep_results(sub, corpus)  # a keep ends the splice's flags
    with pytest.raises(K.KpeError) as e:
        engine.spliced_rows(corpus)
    assert e.value.status == KPE_E_STATE
    engine.drop_results(corpus)
    assert engine.kept_rule_names(corpus) is None
