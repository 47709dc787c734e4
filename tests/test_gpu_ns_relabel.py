"""Namespace label changes on a resident corpus (kpe_corpus_set_namespace_labels) on the device:
after the call every consumer behaves as on a corpus flattened from the same NDJSON with the
resulting table. The oracle (oracle.validate(..., ns_labels=...)) is the reference throughout; a
fresh Corpus(nd, L1) is the second one where the issue is equality with a rebuild."""
import copy
import ctypes
import json

import numpy as np
import pytest

import kyverno_amd as K
from kyverno_amd._lib import load
from kyverno_amd.scan import _key
from tests.policies import c4_policy_set, pss_policy, restricted_latest

pytestmark = pytest.mark.gpu

E_STATE = 5
SEED = 0x4E5


@pytest.fixture(scope="module")
def engine():
    return K.Engine(ordinal=0)


def derive(L0):
    """L1 from L0: values changed in a third of the namespaces (to selector values of the C4 set,
    env=staging and team=team-7, among them, and to keys and values no dictionary holds), a tenth
    removed, one namespace no resource uses added."""
    L1 = {}
    for i, (ns, lab) in enumerate(L0.items()):
        if i % 10 == 1:
            continue
        lab = dict(lab)
        if i % 3 == 0:
            lab["env"] = "staging" if i % 6 == 0 else "qa-new"
            if i % 9 == 0:
                lab["team"] = "team-7"
            lab["zone-new"] = f"z{i % 11}"
            if i % 12 == 0:
                lab.pop("region", None)
                lab["pss"] = "restricted"
            if i % 15 == 0:
                lab["region"] = "r-new"
        L1[ns] = lab
    L1["ns-no-resource-uses"] = {"env": "staging"}
    return L1


def patch_of(old, new):
    p = {ns: lab for ns, lab in new.items() if old.get(ns) != lab or ns not in old}
    p.update({ns: None for ns in old if ns not in new})
    return p


def n_changed(old, new):
    return sum(1 for ns in set(old) | set(new) if (ns in old) != (ns in new) or old.get(ns) != new.get(ns))


@pytest.fixture(scope="module")
def c4_case(oracle):
    """The C4 set over 20000 rows and 10000 namespaces; L0, the derived L1 and, for the namespaces
    that rows use and the table lacks, L2 = L1 with the removed tenth back under other labels."""
    pols = c4_policy_set()
    nd = K.synth_resources(SEED, 20000, mix=3)
    L0 = json.loads(K.synth_ns_labels(SEED, 10000, mix=3))
    L1 = derive(L0)
    L2 = dict(L1)
    L2.update({ns: {"env": ("dev", "prod", "staging")[k % 3], "team": "team-7" if k % 2 else "team-12", "pss": "restricted",
                    "region": "r-back", "back": "again"} for k, ns in enumerate(x for x in L0 if x not in L1)})
    refs = [oracle.validate(pols, nd, ns_labels=L, nthreads=16) for L in (L0, L1, L2)]
    return pols, nd, (L0, L1, L2), refs


def ns_columns(pols):
    """Columns of rules with a namespaceSelector anywhere, and of those the ones whose selector
    builds (sel-ns-bad's `Exists` with values does not: it reads no label, under any table)."""
    cols = [r for r, p in enumerate(pols) if "namespaceSelector" in json.dumps(p)]
    return cols, [r for r in cols if p_name(pols[r]) != "sel-ns-bad"]


def p_name(p):
    return p["metadata"]["name"]


def test_case_is_not_vacuous(c4_case):
    pols, nd, (L0, L1, L2), (r0, r1, r2) = c4_case
    cols, building = ns_columns(pols)
    assert len(cols) == 9 and len(building) == 8
    for r in building:
        assert (r0[:, r] != r1[:, r]).any(), p_name(pols[r])
        assert (r1[:, r] != r2[:, r]).any(), p_name(pols[r])
    other = [r for r in range(len(pols)) if r not in building]
    assert np.array_equal(r0[:, other], r1[:, other])
    used = {json.loads(x)["metadata"]["namespace"] for x in nd.split(b"\n") if x}
    assert any(ns in used for ns in L0 if ns not in L1) and "ns-no-resource-uses" not in used
    assert any("team-7" == v.get("team") for v in L1.values()) and any("staging" == v.get("env") for v in L1.values())


def same_everywhere(engine, ps, c, fresh, ref):
    """Matrix, counts and namespace counts of the relabelled corpus: the oracle's, and a fresh corpus's."""
    v, _, cnt = engine.evaluate(ps, c)
    bad = np.argwhere(v != ref)
    assert bad.size == 0, f"{len(bad)} cells differ from the oracle, first {bad[:5].tolist()}"
    vf, _, cntf = engine.evaluate(ps, fresh)
    assert np.array_equal(vf, ref) and cnt == cntf
    t = engine.namespace_counts(ps, c)
    assert c.namespaces == fresh.namespaces
    assert np.array_equal(t, engine.namespace_counts(ps, fresh))
    assert np.array_equal(t, K.namespace_counts(ps, fresh, ref))


@pytest.mark.parametrize("form", ["patch", "replace"])
def test_equivalence_with_oracle_and_rebuild(engine, c4_case, form):
    pols, nd, (L0, L1, L2), (r0, r1, r2) = c4_case
    ps = K.PolicySet(pols)
    c = K.Corpus(nd, L0)
    v, _, _ = engine.evaluate(ps, c)
    assert np.array_equal(v, r0)
    G, rows = c.namespaces, c.row_namespaces()
    for old, new, ref in ((L0, L1, r1), (L1, L2, r2)):
        n = engine.set_namespace_labels(c, new if form == "replace" else patch_of(old, new), replace=form == "replace")
        assert n == n_changed(old, new) >= 1000
        assert c.namespace_labels() == new
        assert c.namespaces == G and np.array_equal(c.row_namespaces(), rows)
        same_everywhere(engine, ps, c, K.Corpus(nd, new), ref)


@pytest.mark.parametrize("copies", [1, 9])
def test_both_term_forms(engine, oracle, copies):
    """The requirement-mask form (T_NSSELQ: 8 namespaceSelector requirements) and, past 64
    requirements, the selector-record form (T_NSSELECTOR) read the new table."""
    pols = []
    for k in range(copies):
        for p in c4_policy_set():
            q = copy.deepcopy(p)
            q["metadata"]["name"] += f"-{k}"
            pols.append(q)
    nd = K.synth_resources(0x5E1 + copies, 8192, mix=3)
    L0 = json.loads(K.synth_ns_labels(0x5E1, 10000, mix=3))
    L1 = derive(L0)
    ps = K.PolicySet(pols)
    c = K.Corpus(nd, L0)
    ref0, ref1 = (oracle.validate(pols, nd, ns_labels=L, nthreads=16) for L in (L0, L1))
    assert np.array_equal(engine.evaluate(ps, c)[0], ref0) and (ref0 != ref1).any()
    assert engine.set_namespace_labels(c, patch_of(L0, L1)) == n_changed(L0, L1)
    bad = np.argwhere(engine.evaluate(ps, c)[0] != ref1)
    assert bad.size == 0, f"{len(bad)} mismatching cells, first {bad[:5].tolist()}"


def edge_ndjson(n):
    """n rows: C4-mix Deployments and Services with a cluster-scoped row and a Namespace object among
    them; one row: a Deployment in a namespace of its own."""
    ns_obj = {"apiVersion": "v1", "kind": "Namespace", "metadata": {"name": "ns-00003", "labels": {"team": "team-12"}}}
    pv = {"apiVersion": "apps/v1", "kind": "Deployment", "metadata": {"name": "no-namespace", "labels": {"k4": "v1"}},
          "spec": {"template": {"spec": {"containers": [{"name": "c", "image": "x"}]}}}}
    if n == 1:
        pv["metadata"]["namespace"] = "ns-one-row"
        return json.dumps(pv).encode()
    rows = K.synth_resources(0xED6E + n, n - 2, mix=3).split(b"\n")
    rows = [x for x in rows if x]
    rows.insert(len(rows) // 2, json.dumps(pv).encode())
    rows.append(json.dumps(ns_obj).encode())
    assert len(rows) == n
    return b"\n".join(rows)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4096 + 37])
def test_remap_kernel_edges(engine, oracle, n):
    """Row counts around the block size and a partial last block; a corpus flattened with no table
    and then given one; the table emptied again; rows without a namespace; always the oracle."""
    pols = c4_policy_set()
    ps = K.PolicySet(pols)
    nd = edge_ndjson(n)
    L = json.loads(K.synth_ns_labels(0xED6E, 10000, mix=3))
    L[""] = {"team": "team-1x", "env": "prod"}  # an entry under the name cluster-scoped rows carry
    L["ns-one-row"] = {"team": "team-7", "env": "prod"}
    c = K.Corpus(nd)
    assert c.n == n and c.namespace_labels() == {}
    ref_none = oracle.validate(pols, nd, nthreads=8)
    ref_L = oracle.validate(pols, nd, ns_labels=L, nthreads=8)
    assert np.array_equal(engine.evaluate(ps, c)[0], ref_none)
    assert (ref_none != ref_L).any()
    assert engine.set_namespace_labels(c, L) == len(L)
    assert np.array_equal(engine.evaluate(ps, c)[0], ref_L)
    assert np.array_equal(engine.evaluate(ps, K.Corpus(nd, L))[0], ref_L)
    assert engine.set_namespace_labels(c, {}, replace=True) == len(L)
    assert np.array_equal(engine.evaluate(ps, c)[0], ref_none)
    # absent and present without labels: the same to every consumer
    assert engine.set_namespace_labels(c, {ns: {} for ns in list(L)[:500]}) == 500
    assert np.array_equal(engine.evaluate(ps, c)[0], ref_none)
    assert np.array_equal(ref_none, oracle.validate(pols, nd, ns_labels={ns: {} for ns in list(L)[:500]}, nthreads=8))


def test_paths_that_do_not_read_the_table(engine, oracle):
    """A kind-only podSecurity program (the LEAN scan) in one batch launch over three corpora, one
    of them relabelled (its binding was invalidated): all three equal the oracle."""
    pols = [restricted_latest()]
    ps = K.PolicySet(pols)
    L = {"ns-0001": {"env": "prod"}, "ns-0002": {"env": "dev"}}
    nds = [K.synth_resources(0x1EA0 + k, 5000 + 64 * k + k, mix=0) for k in range(3)]
    cs = [K.Corpus(nd, L).upload(engine.device) for nd in nds]
    refs = [oracle.validate(pols, nd, ns_labels=L, nthreads=8) for nd in nds]
    engine.evaluate_batch_async(ps, cs)
    for c, ref in zip(cs, refs):
        assert np.array_equal(engine.fetch(ps, c)[0], ref)
    assert engine.set_namespace_labels(cs[1], {"ns-0001": {"env": "qa", "brand": "new"}, "ns-0003": {"a": "b"}}) == 2
    with pytest.raises(K.KpeError) as e:
        engine.fetch(ps, cs[1])
    assert e.value.status == E_STATE
    engine.evaluate_batch_async(ps, cs)
    for c, ref in zip(cs, refs):
        assert np.array_equal(engine.fetch(ps, c)[0], ref)


def test_policy_exception_with_namespace_selector(engine, oracle):
    pol = pss_policy("restricted", "restricted", "latest", kinds=("Pod", "Deployment"))
    exc = {"apiVersion": "kyverno.io/v2beta1", "kind": "PolicyException", "metadata": {"name": "exempt", "namespace": "kyverno"},
           "spec": {"exceptions": [{"policyName": p_name(pol), "ruleNames": ["restricted"]}],
                    "match": {"any": [{"resources": {"namespaceSelector": {"matchLabels": {"exempt": "yes"}}}}]}}}
    nd = K.synth_resources(0xE8C, 6000, mix=K.SYNTH_MIXED)
    names = sorted({json.loads(x).get("metadata", {}).get("namespace", "") for x in nd.split(b"\n") if x} - {""})
    L0 = {ns: {"exempt": "yes" if i % 4 == 0 else "no"} for i, ns in enumerate(names)}
    L1 = {ns: {"exempt": "yes" if i % 4 == 1 else "no"} for i, ns in enumerate(names)}
    ps = K.PolicySet([pol], [exc])
    ref0, ref1 = (oracle.validate([pol], nd, ns_labels=L, nthreads=8, exceptions=[exc]) for L in (L0, L1))
    flips = (ref0 != ref1)
    assert flips.sum() > 100 and ((ref0 == 5) & flips).any() and ((ref1 == 5) & flips).any()  # skipped by the exception
    c = K.Corpus(nd, L0)
    assert np.array_equal(engine.evaluate(ps, c)[0], ref0)
    assert engine.set_namespace_labels(c, L1, replace=True) == n_changed(L0, L1)
    assert np.array_equal(engine.evaluate(ps, c)[0], ref1)


@pytest.mark.parametrize("keep", ["matrix", "fingerprints"])
def test_results_side(engine, c4_case, keep):
    """Kept results under L0, relabel, evaluate: the changed rows are exactly the rows whose oracle
    rows differ; retired rows stay NA; no fetch between the relabel and the evaluation; the call
    refuses an uploaded corpus without its device and changes nothing."""
    pols, nd, (L0, L1, _), (r0, r1, _) = c4_case
    ps = K.PolicySet(pols)
    L = load()
    c = K.Corpus(nd, L0).upload(engine.device)
    diff = np.flatnonzero((r0 != r1).any(axis=1))
    retired = np.concatenate([diff[:40:2], np.array([0, 1, c.n - 1])]).astype(np.uint64)
    engine.retire_rows(c, retired)
    ret = set(int(x) for x in retired)
    engine.evaluate_async(ps, c)
    if keep == "matrix":
        engine.keep_results(ps, c)
    else:
        engine.keep_fingerprints(ps, c)
    # an uploaded corpus: a null device (and another device, where there is one) is refused
    js = json.dumps(patch_of(L0, L1)).encode()
    n = ctypes.c_uint64(0)
    assert L.kpe_corpus_set_namespace_labels(None, c.h, js, len(js), 0, ctypes.byref(n)) == E_STATE
    import torch
    if torch.cuda.device_count() > 1:
        other = K.Device(1)
        assert L.kpe_corpus_set_namespace_labels(other.h, c.h, js, len(js), 0, ctypes.byref(n)) == E_STATE
    assert c.namespace_labels() == L0
    assert np.array_equal(engine.fetch(ps, c)[0][sorted(set(range(c.n)) - ret)], r0[sorted(set(range(c.n)) - ret)])
    # nothing really changes: nothing is invalidated
    assert engine.set_namespace_labels(c, {ns: L0[ns] for ns in list(L0)[:50]}) == 0
    engine.fetch(ps, c)
    assert engine.set_namespace_labels(c, patch_of(L0, L1)) == n_changed(L0, L1)
    for call in (lambda: engine.fetch(ps, c), lambda: engine.select_cells(ps, c, K.SEL(2)),
                 lambda: engine.row_summaries(ps, c), lambda: engine.namespace_counts(ps, c),
                 lambda: engine.changed_rows(ps, c) if keep == "matrix" else engine.changed_rows_fp(ps, c)):
        with pytest.raises(K.KpeError) as e:
            call()
        assert e.value.status == E_STATE
    assert np.array_equal(engine.retired_rows(c), np.unique(retired))
    engine.evaluate_async(ps, c)
    want = sorted(set(diff.tolist()) - ret)
    if keep == "matrix":
        rows, vr, total = engine.changed_rows(ps, c)
    else:
        rows, vr, _, total = engine.changed_rows_fp(ps, c)
    assert rows.tolist() == want and total == len(want) > 100
    assert np.array_equal(vr, r1[want])
    v = engine.fetch(ps, c)[0]
    assert not v[sorted(ret)].any()
    live = sorted(set(range(c.n)) - ret)
    assert np.array_equal(v[live], r1[live])


# ---- the scanner ----
def enc(d):
    return json.dumps(d, separators=(",", ":")).encode()


class World:
    """Resources by logical row (None: deleted), the namespace labels, and the oracle's matrix."""

    def __init__(self, oracle, pols, docs, labels):
        self.oracle, self.pols, self.cur, self.labels = oracle, pols, list(docs), dict(labels)

    def live(self):
        return [i for i, d in enumerate(self.cur) if d is not None]

    def ndjson(self):
        return b"\n".join(enc(self.cur[i]) for i in self.live())

    def matrix(self):
        out = np.zeros((len(self.cur), len(self.pols)), dtype=np.uint8)
        out[self.live()] = self.oracle.validate(self.pols, self.ndjson(), ns_labels=self.labels, nthreads=8)
        return out


def check_rows(got, before, after, deleted=()):
    if before.shape[0] < after.shape[0]:
        before = np.vstack([before, np.zeros((after.shape[0] - before.shape[0], before.shape[1]), dtype=np.uint8)])
    want = set(np.flatnonzero((before != after).any(axis=1)).tolist()) | set(deleted)
    assert set(got) == want, (sorted(set(got) - want)[:8], sorted(want - set(got))[:8])
    for l, row in got.items():
        assert row is None if l in deleted else np.array_equal(row, after[l]), l


def check_ns_counts(sc, world, ps, m):
    names, counts = sc.namespace_counts()
    fresh = K.Corpus(world.ndjson(), world.labels)
    want = dict(zip(fresh.namespaces, K.namespace_counts(ps, fresh, m[world.live()])))
    assert len(set(names)) == len(names) and set(want) <= set(names)
    for nm, t in zip(names, counts):
        assert np.array_equal(t, want.get(nm, np.zeros_like(t))), nm
    tot = sc.cli_summary(True)
    assert tot == K.cli_summary_ns(ps, fresh, K.namespace_counts(ps, fresh, m[world.live()]), True)


@pytest.mark.parametrize("keep", ["matrix", "fingerprints"])
def test_scanner(engine, oracle, keep):
    pols = c4_policy_set()
    pols[15]["spec"]["validationFailureActionOverrides"] = [
        {"action": "Enforce", "namespaceSelector": {"matchLabels": {"env": "staging"}}}]
    ps = K.PolicySet(pols)
    docs = []
    for i, line in enumerate(K.synth_resources(0x5CA, 3000, mix=3).strip(b"\n").split(b"\n")):
        d = json.loads(line)
        d["metadata"]["uid"] = f"uid-{i}"
        docs.append(d)
    L0 = json.loads(K.synth_ns_labels(0x5CA, 10000, mix=3))
    w = World(oracle, pols, docs, L0)
    sc = K.ResidentScanner(engine, w.ndjson(), ns_labels=L0, keep=keep, keyed=True, ns_objects=True)
    assert sc.set_namespace_labels({"ns-00000": {"env": "none-yet"}}) == {} and sc.last_stats["relabelled"] == 1
    w.labels["ns-00000"] = {"env": "none-yet"}
    m = w.matrix()
    got = sc.apply(ps)
    assert set(got) == set(np.flatnonzero(m.any(axis=1)).tolist()) and np.array_equal(sc.matrix(), m)

    def edited(i, k):
        d = copy.deepcopy(w.cur[i])
        d["metadata"].setdefault("labels", {})["k8"] = f"v{k % 3}"
        w.cur[i] = d
        return d

    # two delta segments and retired rows: edits, a new resource, a delete
    new = json.loads(K.synth_resources(0x5CB, 1, mix=3, first_index=5000))
    new["metadata"]["uid"] = "new-0"
    ups = [edited(i, i) for i in (3, 50, 51)] + [new]
    w.cur.append(new)
    w.cur[7] = None
    got = sc.update(b"\n".join(enc(d) for d in ups), [7])
    m2 = w.matrix()
    check_rows(got, m, m2, {7})
    got = sc.update(enc(edited(50, 1)) + b"\n" + enc(edited(900, 2)))
    m3 = w.matrix()
    check_rows(got, m2, m3)
    assert len(sc._segs) == 3 and np.array_equal(sc.matrix(), m3)
    check_ns_counts(sc, w, ps, m3)

    # the relabel: exactly the rows whose oracle row differs, across the segments
    before = dict(w.labels)
    L1 = derive(before)
    w.labels = dict(L1)
    m4 = w.matrix()
    edits = dict(sc.edits)
    got = sc.set_namespace_labels(patch_of(before, L1))
    check_rows(got, m3, m4)
    assert len(got) > 50 and sc.last_stats["relabelled"] == n_changed(before, L1)
    assert sc.last_stats["changed"] == len(got) and sc.edits == edits
    live = w.live()
    assert np.array_equal(sc.matrix()[live], m4[live]) and not sc.matrix()[7].any()
    assert sc.apply(ps) == {}  # the result was kept
    assert sc.set_namespace_labels(L1, replace=True) == {} and sc.last_stats == {"relabelled": 0, "changed": 0}
    check_ns_counts(sc, w, ps, m4)

    # a new resource in a relabelled namespace is judged under L1
    ns_env = next(ns for ns, lab in L1.items() if ns in L0 and lab.get("env") == "staging" and L0[ns].get("env") != "staging")
    fresh = copy.deepcopy(next(d for d in w.cur if d is not None and d["kind"] == "Deployment"))
    fresh["metadata"].update(uid="new-1", name="in-relabelled", namespace=ns_env)
    w.cur.append(fresh)
    got = sc.update(enc(fresh))
    m5 = w.matrix()
    check_rows(got, m4, m5)
    assert np.array_equal(sc.matrix(), m5)

    # Namespace objects as label events: an upsert, then a delete
    target = fresh["metadata"]["namespace"]
    nsobj = {"apiVersion": "v1", "kind": "Namespace", "metadata": {"name": target, "uid": "ns-obj", "labels": {
        "env": "prod", "team": "team-7", "count": 3}}}
    w.cur.append(nsobj)
    w.labels[target] = {"env": "prod", "team": "team-7"}
    moved = edited(3, 2)
    got = sc.update(enc(nsobj) + b"\n" + enc(moved))
    m6 = w.matrix()
    check_rows(got, m5, m6)
    assert sc.last_stats["relabelled"] == 1 and len(w.cur) - 2 in got  # the resource in that namespace
    assert np.array_equal(sc.matrix(), m6)
    w.cur[-1] = None
    del w.labels[target]
    got = sc.update(b"", [_key(enc(nsobj), 0)])
    m7 = w.matrix()
    check_rows(got, m6, m7, {len(w.cur) - 1})
    assert sc.last_stats["relabelled"] == 1 and np.array_equal(sc.matrix(), m7)
    check_ns_counts(sc, w, ps, m7)

    # compact keeps the table
    sc.compact()
    assert len(sc._segs) == 1 and sc.corpus.namespace_labels() == w.labels
    assert np.array_equal(sc.matrix(), m7) and sc.apply(ps) == {}
    check_ns_counts(sc, w, ps, m7)


@pytest.mark.parametrize("keep", ["matrix", "fingerprints"])
def test_scanner_not_keyed(engine, c4_case, keep):
    pols, nd, (L0, L1, _), (r0, r1, _) = c4_case
    ps = K.PolicySet(pols)
    sc = K.ResidentScanner(engine, nd, ns_labels=L0, keep=keep)
    assert sc.set_namespace_labels({"ns-no-resource-uses": {"a": "b"}}) == {}
    got = sc.apply(ps)
    assert set(got) == set(np.flatnonzero(r0.any(axis=1)).tolist())
    got = sc.set_namespace_labels(L1, replace=True)
    want = np.flatnonzero((r0 != r1).any(axis=1))
    assert sorted(got) == want.tolist() and all(np.array_equal(got[int(i)], r1[i]) for i in want)
    assert sc.last_stats["changed"] == len(want) and sc.apply(ps) == {}
    names, counts = sc.namespace_counts()
    assert names == sc.corpus.namespaces and np.array_equal(counts, K.namespace_counts(ps, sc.corpus, r1))
