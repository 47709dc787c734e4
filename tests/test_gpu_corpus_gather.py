"""Compaction by gather on the device: a corpus gathered from rows of other corpora
(kpe_corpus_gather) evaluates cell for cell like a fresh flatten of the same lines, kept matrices and
fingerprints are carried over by kpe_results_gather, and ResidentScanner.compact() by gather is
indistinguishable from compact(reflatten=True) while it compiles and evaluates nothing. Both sides
of every comparison run through the engine; the existing suites pin a fresh flatten to the oracle."""
import copy
import json
import random

import numpy as np
import pytest

import kyverno_amd as K
from kyverno_amd._lib import load
from tests.policies import (_golden, cond_policy_set, parity_policy_set, pss_policy, restricted_latest, selector_policy,
                            var_policy_set)

pytestmark = pytest.mark.gpu

E_INVALID, E_STATE = 1, 5
PASS, FAIL, SKIP = 1, 2, 5
LEAN6 = 7
SIZES = [1, 64, 129, 700]
NO_AUTOGEN = {"pod-policies.kyverno.io/autogen-controllers": "none"}


@pytest.fixture(scope="module")
def engine():
    return K.Engine(ordinal=0)


def enc(d):
    return json.dumps(d, separators=(",", ":")).encode()


def _pod_specs(d):
    spec = d.get("spec")
    for path in ((), ("template", "spec"), ("jobTemplate", "spec", "template", "spec")):
        s = spec
        for k in path:
            s = s.get(k) if isinstance(s, dict) else None
        if isinstance(s, dict):
            yield s


def _own(d, t):
    """Resource d as source t holds it: namespaces and images no other source uses."""
    d = copy.deepcopy(d)
    meta = d.setdefault("metadata", {})
    if isinstance(meta.get("namespace"), str):
        meta["namespace"] = f"s{t}-{meta['namespace']}"
    for s in _pod_specs(d):
        for key in ("containers", "initContainers", "ephemeralContainers"):
            for c in s.get(key) or []:
                if isinstance(c, dict) and isinstance(c.get("image"), str):
                    c["image"] = f"r{t}.example/{c['image']}"
    return d


@pytest.fixture(scope="module")
def case(engine):
    """Four sources of 1, 64, 129 and 700 rows (pods, workloads, services: the mixed and the fan-out
    synthetic shapes, interleaved), disjoint in namespaces and images, a label table over all their
    namespaces, rows retired in the two larger ones, and the live rows in shuffled order
    (random.Random(11))."""
    a = [json.loads(x) for x in K.synth_resources(0x6A, 450, mix=K.SYNTH_MIXED).split(b"\n") if x.strip()]
    b = [json.loads(x) for x in K.synth_resources(0x6B, 444, mix=K.SYNTH_FANOUT).split(b"\n") if x.strip()]
    docs = [x for pair in zip(a, b) for x in pair] + a[len(b):]
    assert len(docs) == sum(SIZES)
    # the one row of source 0 is a Pod, so that source shows in every program
    first = next(i for i, d in enumerate(docs) if d["kind"] == "Pod")
    docs[0], docs[first] = docs[first], docs[0]
    lines, at = [], 0
    for t, n in enumerate(SIZES):
        lines.append([enc(_own(d, t)) for d in docs[at:at + n]])
        at += n
    names = sorted({json.loads(x)["metadata"].get("namespace", "") for src in lines for x in src} - {""})
    assert all(len({n for n in names if n.startswith(f"s{t}-")}) > 0 for t in range(4))
    labels = {ns: {"env": ("prod", "dev", "staging")[i % 3], "exempt": "yes" if i % 4 == 0 else "no"}
              for i, ns in enumerate(names)}
    srcs = [K.Corpus(b"\n".join(src), labels).upload(engine.device) for src in lines]
    assert [s.n for s in srcs] == SIZES
    retired = {2: [0, 63, 64, 128], 3: list(range(5, 700, 9))}
    for t, rows in retired.items():
        engine.retire_rows(srcs[t], rows)
    pairs = [(t, r) for t, n in enumerate(SIZES) for r in range(n) if r not in retired.get(t, ())]
    random.Random(11).shuffle(pairs)
    assert {t for t, _ in pairs} == {0, 1, 2, 3}  # every source contributes a row
    fresh_nd = b"\n".join(lines[t][r] for t, r in pairs)
    return srcs, pairs, labels, fresh_nd, lines


def program(name):
    if name == "lean":  # kind-only restricted:latest
        return K.PolicySet([restricted_latest()])
    if name == "tape":  # the chart's pattern, deny and foreach rules, the condition and the variable sets
        chart = _golden("chart_policies.json")
        return K.PolicySet(chart["baseline"] + chart["restricted"] + cond_policy_set() + var_policy_set())
    if name == "selectors":  # selectors under namespace labels, an exception, a podSecurity.exclude
        kinds = ("Pod", "Deployment")
        pols = [selector_policy("ns-prod", kinds=kinds, ns_selector={"matchLabels": {"env": "prod"}}),
                selector_policy("ns-notin", kinds=("*",), ns_selector={"matchExpressions": [
                    {"key": "env", "operator": "NotIn", "values": ["dev"]}]}),
                selector_policy("tier", kinds=kinds, selector={"matchLabels": {"tier": "front*"}},
                                exclude={"any": [{"resources": {"namespaceSelector": {"matchLabels": {"env": "staging"}}}}]}),
                pss_policy("x-caps", "baseline", kinds=kinds, exclude=[{"controlName": "Capabilities", "images": ["r3.example/*"]}]),
                pss_policy("x-ports", "baseline", kinds=kinds, exclude=[{"controlName": "Host Ports", "images": ["*"]},
                                                                        {"controlName": "Host Namespaces"}]),
                pss_policy("restricted", "restricted", "latest", kinds=kinds)]
        exc = {"apiVersion": "kyverno.io/v2beta1", "kind": "PolicyException", "metadata": {"name": "exempt", "namespace": "kyverno"},
               "spec": {"exceptions": [{"policyName": "pol-restricted", "ruleNames": ["restricted", "autogen-restricted"]}],
                        "match": {"any": [{"resources": {"namespaceSelector": {"matchLabels": {"exempt": "yes"}}}}]}}}
        return K.PolicySet(pols, [exc])
    raise KeyError(name)


def test_gathered_corpus_evaluates_like_a_fresh_flatten(engine, case):
    srcs, pairs, labels, fresh_nd, _ = case
    g = K.Corpus.gather(srcs, pairs).upload(engine.device)
    fresh = K.Corpus(fresh_nd, labels).upload(engine.device)
    assert g.n == fresh.n == len(pairs)
    assert not engine.retired_rows(g).size and engine.kept_results(g) is None and engine.kept_fingerprints(g, 0, 0) is None
    seen = set()
    for name in ("lean", "tape", "selectors"):
        ps = program(name)
        vg, mg, cg = engine.evaluate(ps, g, check_masks=True)
        if name == "lean":  # the LEAN forms: without masks too
            assert load().kpe_debug_lean_kind(g.h, 0) == LEAN6
            engine.evaluate_async(ps, g)
            assert load().kpe_debug_lean_form(engine.device.h) >= 0
            assert np.array_equal(engine.fetch(ps, g)[0], vg)
        vf, mf, cf = engine.evaluate(ps, fresh, check_masks=True)
        bad = np.argwhere(vg != vf)
        assert bad.size == 0, (name, len(bad), bad[:5].tolist(), [pairs[i] for i in bad[:5, 0]])
        assert np.array_equal(engine.cv_masks(ps, g, raw=True), engine.cv_masks(ps, fresh, raw=True)), name
        assert np.array_equal(mg, mf) and cg == cf, name
        assert np.array_equal(engine.namespace_counts(ps, g)[[g.namespaces.index(n) for n in fresh.namespaces]],
                              engine.namespace_counts(ps, fresh)), name
        seen |= set(np.unique(vg).tolist())
        if name == "lean":
            for t in range(4):  # every source's rows have responses
                assert vg[[i for i, (s, _) in enumerate(pairs) if s == t]].any(), t
    assert {PASS, FAIL, SKIP} <= seen


def _rules(R):
    """A PolicySet of exactly R podSecurity rules over Pods."""
    levels = [("baseline", "latest"), ("restricted", "latest"), ("baseline", "v1.19"), ("restricted", "v1.24"), ("privileged", "latest")]
    pols = []
    for r in range(R):
        p = pss_policy(f"r{r}", *levels[r % len(levels)])
        p["metadata"]["annotations"] = dict(NO_AUTOGEN)
        if r % 7 == 3:  # match-only variety: a few rules that select by name
            p["spec"]["rules"][0]["match"]["any"][0]["resources"]["names"] = [f"*{r % 10}"]
        pols.append(p)
    ps = K.PolicySet(pols)
    assert ps.num_rules == R
    return ps


@pytest.mark.parametrize("keep", ["matrix", "fingerprints"])
def test_kept_results_are_carried_over(engine, case, keep):
    srcs0, pairs, labels, _, lines = case
    srcs = [K.Corpus(b"\n".join(src), labels).upload(engine.device) for src in lines]  # this test's own: it keeps on them
    for s, s0 in zip(srcs, srcs0):
        engine.retire_rows(s, engine.retired_rows(s0))
    P = parity_policy_set()
    A, B = K.PolicySet(P[:6]), K.PolicySet(P[2:9])
    for s in srcs:
        engine.evaluate_async(A, s)
        if keep == "matrix":
            engine.keep_results(A, s)
        else:
            engine.keep_fingerprints(A, s)
    g = K.Corpus.gather(srcs, pairs).upload(engine.device)
    engine.gather_results(g, srcs, pairs)
    if keep == "matrix":
        host = [engine.kept_results(s) for s in srcs]
        want = np.array([host[t][r] for t, r in pairs], dtype=np.uint8)
        assert engine.kept_rule_names(g) == A.rule_names and engine.kept_fingerprints(g, 0, 0) is None
        assert np.array_equal(engine.kept_results(g), want) and want.any()
        engine.evaluate_async(B, g)
        rows, vr, total = engine.changed_rows(B, g)
        vB = engine.fetch(B, g)[0]
        hrows, hvr, htotal = K.changed_rows(want, vB, K.column_map(A.rule_names, B.rule_names))
        assert total == htotal > 0 and np.array_equal(rows, hrows) and np.array_equal(vr, hvr)
        # explicit kinds: the matrix alone is there
        engine.gather_results(g, srcs, pairs, K.GATHER_MATRIX)
        assert np.array_equal(engine.kept_results(g), want)
        with pytest.raises(K.KpeError) as e:
            engine.gather_results(g, srcs, pairs, K.GATHER_FINGERPRINTS)
        assert e.value.status == E_STATE
    else:
        host = [engine.kept_fingerprints(s) for s in srcs]
        want = np.array([host[t][r] for t, r in pairs], dtype=np.uint64)
        assert engine.kept_results(g) is None
        assert np.array_equal(engine.kept_fingerprints(g), want) and want.any()
        engine.evaluate_async(B, g)
        rows, vr, fps, total = engine.changed_rows_fp(B, g)
        vB = engine.fetch(B, g)[0]
        new = K.row_fingerprints(vB, K.rule_salts(B))
        hrows = K.changed_fingerprints(want, new)
        assert total == len(hrows) > 0 and np.array_equal(rows, hrows)
        assert np.array_equal(vr, vB[hrows.astype(np.int64)]) and np.array_equal(fps, new[hrows.astype(np.int64)])
        with pytest.raises(K.KpeError) as e:
            engine.gather_results(g, srcs, pairs, K.GATHER_MATRIX)
        assert e.value.status == E_STATE


@pytest.mark.parametrize("R", [1, 3, 5, 204])
def test_edge_shapes(engine, case, R):
    """Rows of R = 1, 3, 5 and 204 bytes, lists of 1, 65 and every live row, a source no pair names
    that keeps nothing, both kinds at once."""
    _, _, labels, _, lines = case
    srcs = [K.Corpus(b"\n".join(src), labels).upload(engine.device) for src in lines]
    ps = _rules(R)
    for s in srcs[:3]:  # source 3 keeps nothing
        engine.evaluate_async(ps, s)
        engine.keep_results(ps, s)
        engine.keep_fingerprints(ps, s)
    host = [engine.kept_results(s) for s in srcs[:3]]
    fps = [engine.kept_fingerprints(s) for s in srcs[:3]]
    rng = random.Random(R)
    full = [(t, r) for t in range(3) for r in range(SIZES[t])]
    rng.shuffle(full)
    for pairs in ([(2, 128)], [(rng.randrange(1, 3), rng.randrange(64)) for _ in range(64)] + [(0, 0)], full):
        g = K.Corpus.gather(srcs, pairs).upload(engine.device)
        engine.gather_results(g, srcs, pairs)
        want = np.array([host[t][r] for t, r in pairs], dtype=np.uint8).reshape(len(pairs), R)
        assert np.array_equal(engine.kept_results(g), want), (R, len(pairs))
        assert np.array_equal(engine.kept_fingerprints(g), np.array([fps[t][r] for t, r in pairs], dtype=np.uint64))
        assert engine.kept_rule_names(g) == ps.rule_names
    assert any(h.any() for h in host)
    # a row of the source that keeps nothing: nothing to carry with what=0, KPE_E_STATE when asked for
    pairs = [(3, 1), (1, 2)]
    g = K.Corpus.gather(srcs, pairs).upload(engine.device)
    engine.gather_results(g, srcs, pairs)
    assert engine.kept_results(g) is None and engine.kept_fingerprints(g, 0, 0) is None
    for what in (K.GATHER_MATRIX, K.GATHER_FINGERPRINTS, K.GATHER_MATRIX | K.GATHER_FINGERPRINTS):
        with pytest.raises(K.KpeError) as e:
            engine.gather_results(g, srcs, pairs, what)
        assert e.value.status == E_STATE


def test_state_and_argument_errors(engine, case):
    _, _, labels, _, lines = case
    a = K.Corpus(b"\n".join(lines[1]), labels).upload(engine.device)
    b = K.Corpus(b"\n".join(lines[2]), labels).upload(engine.device)
    A, B = _rules(3), _rules(5)
    for c, ps in ((a, A), (b, B)):
        engine.evaluate_async(ps, c)
        engine.keep_results(ps, c)
    pairs = [(0, 1), (1, 2)]
    g = K.Corpus.gather([a, b], pairs)

    def status(*args, **kw):
        with pytest.raises(K.KpeError) as e:
            engine.gather_results(*args, **kw)
        return e.value.status

    assert status(g, [a, b], pairs) == E_STATE  # dst is not uploaded
    g.upload(engine.device)
    assert status(g, [a, b], pairs) == E_STATE  # the kept names disagree (3 rules against 5)
    same = [(0, 1), (0, 2)]
    g2 = K.Corpus.gather([a, b], same).upload(engine.device)
    engine.gather_results(g2, [a, b], same)  # b is listed for no row: its names do not count
    assert engine.kept_rule_names(g2) == A.rule_names
    host_only = K.Corpus(b"\n".join(lines[2]), labels)
    assert status(g2, [a, host_only], same) == E_STATE  # a source that is not on the device
    # renamed rules of the same count
    p = pss_policy("other", "baseline")
    p["metadata"]["annotations"] = dict(NO_AUTOGEN)
    C = K.PolicySet([p] + [pss_policy(f"r{r}", "baseline") | {"metadata": {"name": f"pol-r{r}", "annotations": dict(NO_AUTOGEN)}}
                           for r in (1, 2)])
    assert C.num_rules == 3 and C.rule_names != A.rule_names
    engine.evaluate_async(C, b)
    engine.keep_results(C, b)
    assert status(g, [a, b], pairs) == E_STATE
    # arguments: the row count, dst among the sources, a pair outside, a retired row, an unknown kind
    assert status(g, [a, b], same + [(0, 3)]) == E_INVALID
    assert status(a, [a, b], [(0, r) for r in range(a.n)]) == E_INVALID
    assert status(g, [a, b], [(0, 1), (1, 129)]) == E_INVALID
    assert status(g2, [a, b], same, what=4) == E_INVALID
    engine.retire_rows(a, [2])
    assert status(g2, [a, b], same) == E_INVALID
    assert load().kpe_results_gather(None, g2.h, None, 0, None, 0, 0) == E_INVALID
    assert engine.kept_rule_names(g2) == A.rule_names  # untouched by the refused calls


# ---- the scanner ----
def with_uids(nd, prefix):
    out = []
    for i, line in enumerate(nd.strip(b"\n").split(b"\n")):
        d = json.loads(line)
        d.setdefault("metadata", {})["uid"] = f"{prefix}-{i}"
        out.append(d)
    return out


def same_rows(got, want):
    assert set(got) == set(want), (sorted(set(got) - set(want))[:8], sorted(set(want) - set(got))[:8])
    for l, row in want.items():
        assert (got[l] is None) if row is None else np.array_equal(got[l], row), l


def same_state(a, b):
    """Matrix, namespace counts, CLI summary and fingerprints. The counts are compared by namespace
    name: group ids follow the dictionaries, and a gathered corpus may keep a group without rows (all
    zeros) where a fresh flatten has none (include/kpe.h, kpe_corpus_gather)."""
    assert np.array_equal(a.matrix(), b.matrix())
    (na, ca), (nb, cb) = a.namespace_counts(), b.namespace_counts()
    assert len(set(na)) == len(na) and len(set(nb)) == len(nb) and ca.shape[1:] == cb.shape[1:]
    ta, tb = dict(zip(na, ca)), dict(zip(nb, cb))
    zero = np.zeros(ca.shape[1:], dtype=ca.dtype)
    for ns in set(ta) | set(tb):
        assert np.array_equal(ta.get(ns, zero), tb.get(ns, zero)), ns
    assert ca.any() and set(tb) <= set(ta)
    assert a.cli_summary() == b.cli_summary()
    fa, fb = a.fingerprints(), b.fingerprints()
    assert (fa is None) == (fb is None)
    if fa is not None:
        assert np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1])


class Reflatten(K.ResidentScanner):
    """The twin: every compaction, `update`'s own included, flattens again."""

    def compact(self, reflatten=False):
        super().compact(reflatten=True)


@pytest.mark.parametrize("keep", ["matrix", "fingerprints"])
def test_scanner_gather_against_reflatten(engine, keep):
    P = copy.deepcopy(parity_policy_set())
    pols = ([restricted_latest()] + P[1:6] +
            [selector_policy("ns-prod", kinds=("Pod",), ns_selector={"matchLabels": {"env": "prod"}})])
    docs = with_uids(K.synth_resources(0x6C, 1500, mix=K.SYNTH_MIXED), "uid")
    nd = b"\n".join(enc(d) for d in docs)
    names = sorted({d["metadata"].get("namespace", "") for d in docs} - {""})
    labels = {ns: {"env": "prod" if i % 2 else "dev"} for i, ns in enumerate(names)}
    sc = K.ResidentScanner(engine, nd, labels, keep=keep, keyed=True, max_segments=2)
    twin = Reflatten(engine, nd, labels, keep=keep, keyed=True, max_segments=2)
    ps = K.PolicySet(pols)
    same_rows(sc.apply(ps), twin.apply(ps))
    pods = [i for i, d in enumerate(docs) if d["kind"] == "Pod"]
    compacted = 0
    for step in range(4):  # every second update crosses max_segments=2
        ups = []
        for i in pods[step * 40:step * 40 + 40:2]:
            d = copy.deepcopy(docs[i])
            d["spec"]["hostNetwork"] = not d["spec"].get("hostNetwork", False)
            docs[i] = d
            ups.append(enc(d))
        new = copy.deepcopy(docs[pods[0]])
        new["metadata"].update(uid=f"new-{step}", name=f"new-{step}")
        ups.append(enc(new))
        dele = [("uid", f"uid-{pods[-1 - step]}")]
        got, want = sc.update(b"\n".join(ups), dele), twin.update(b"\n".join(ups), dele)
        same_rows(got, want)
        assert len(got) > 0 and sc.last_stats == twin.last_stats
        compacted += bool(sc.last_stats.get("compacted"))
        same_state(sc, twin)
    assert compacted == 2 and len(sc._segs) == 1
    # a namespace label change, then (with a kept matrix) an edit of one policy, then compact()
    flip = {ns: {"env": "dev" if lab["env"] == "prod" else "prod"} for ns, lab in list(labels.items())[:7]}
    got, want = sc.set_namespace_labels(flip), twin.set_namespace_labels(flip)
    same_rows(got, want)
    assert len(got) > 0
    if keep == "matrix":
        p2 = copy.deepcopy(pols)
        p2[4]["spec"]["rules"][0]["validate"]["podSecurity"]["version"] = "v1.0"
        got = sc.apply_edit(K.PolicySet(p2), K.PolicySet([p2[4]]))
        want = twin.apply(K.PolicySet(p2), edited={p2[4]["metadata"]["name"]})
        same_rows(got, want)
        assert len(got) > 0
    d = copy.deepcopy(docs[pods[200]])
    d["spec"]["hostPID"] = True
    same_rows(sc.update(enc(d)), twin.update(enc(d)))
    assert len(sc._segs) == 2
    sc.compact()
    twin.compact()
    assert len(sc._segs) == len(twin._segs) == 1 and sc.corpus.n == twin.corpus.n
    assert engine.kept_results(sc.corpus) is None or np.array_equal(engine.kept_results(sc.corpus), engine.kept_results(twin.corpus))
    same_state(sc, twin)
    # and life goes on: the next update compares with the carried results
    ups = []
    for i in pods[300:340]:
        d = copy.deepcopy(docs[i])
        d["spec"]["hostNetwork"] = not d["spec"].get("hostNetwork", False)
        ups.append(enc(d))
    got, want = sc.update(b"\n".join(ups)), twin.update(b"\n".join(ups))
    same_rows(got, want)
    assert len(got) > 0
    same_state(sc, twin)


def test_compact_leaves_a_lazy_policy_set_alone(engine):
    pols = [restricted_latest(), pss_policy("b", "baseline")]
    docs = with_uids(K.synth_resources(0x6D, 300, mix=K.SYNTH_PODS), "uid")
    sc = K.ResidentScanner(engine, b"\n".join(enc(d) for d in docs), keyed=True)
    sc.apply(K.PolicySet(pols))
    d = copy.deepcopy(docs[3])
    d["spec"]["hostNetwork"] = not d["spec"].get("hostNetwork", False)
    sc.update(enc(d), [("uid", "uid-9")])
    before = sc.matrix()
    p2 = copy.deepcopy(pols)
    p2[1]["spec"]["rules"][0]["validate"]["podSecurity"]["version"] = "v1.0"
    calls = []

    def full():
        calls.append(1)
        raise AssertionError("compact() resolved the lazy PolicySet")

    sc.apply_edit(full, K.PolicySet([p2[1]]))
    sc.compact()
    assert not calls and len(sc._segs) == 1
    kept = engine.kept_results(sc.corpus)
    assert kept is not None and kept.shape == (sc.corpus.n, K.PolicySet(p2).num_rules)
    # what it carried is the spliced matrix: the rows of a full evaluation of the new set
    live = np.array(sc._map.live())
    want = engine.evaluate(K.PolicySet(p2), K.Corpus(b"\n".join(sc._lines[l] for l in live)))[0]
    assert np.array_equal(kept, want) and before.shape[1] == want.shape[1]
    with pytest.raises(AssertionError):
        sc.matrix()  # a reader that needs the whole set is what resolves it
    assert calls == [1]


def test_loaded_fingerprints_survive_a_compaction_before_the_first_apply(engine):
    """A restart: saved fingerprints are given back, resource events arrive and force a compaction
    before the first apply. The first apply then returns only the rows that really changed, as with
    a scanner that flattens again."""
    pols = [restricted_latest(), pss_policy("b", "baseline")]
    ps = K.PolicySet(pols)
    docs = with_uids(K.synth_resources(0x6E, 600, mix=K.SYNTH_PODS), "uid")
    nd = b"\n".join(enc(d) for d in docs)
    first = K.ResidentScanner(engine, nd, keep="fingerprints", keyed=True)
    assert len(first.apply(ps)) > 100
    saved = first.fingerprints()
    assert saved is not None and saved.shape == (600,) and saved.any()
    sc = K.ResidentScanner(engine, nd, keep="fingerprints", keyed=True, fingerprints=saved, max_segments=1)
    twin = Reflatten(engine, nd, keep="fingerprints", keyed=True, fingerprints=saved, max_segments=1)
    ups = []
    for i in range(10, 50, 2):
        d = copy.deepcopy(docs[i])
        d["spec"]["hostNetwork"] = not d["spec"].get("hostNetwork", False)
        ups.append(enc(d))
    assert sc.update(b"\n".join(ups), [("uid", "uid-7")]) == {} == twin.update(b"\n".join(ups), [("uid", "uid-7")])
    assert sc.last_stats.get("compacted") and len(sc._segs) == 1
    fa, fb = sc.fingerprints(), twin.fingerprints()
    assert fa is not None and np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1])
    got, want = sc.apply(ps), twin.apply(ps)
    same_rows(got, want)
    assert 0 < len(got) <= 20 and set(got) <= set(range(10, 50, 2))  # not every row with a response
