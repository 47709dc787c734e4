"""ResidentScanner.apply_edit against its twin: two keyed scanners with reports over the same 5,000
resources, one driven with apply_edit (the edited policies evaluated alone and spliced into the kept
matrix), the other with apply(full, edited=names) (everything evaluated, compared and kept). Through
edits, an update, an added policy, a namespace label change, a removed policy and a compaction the
two must return the same rows and hold the same matrix, counts and summary, and the entries
reports(rows, policies="edited") renders from the partial evaluation must be the edited policies'
entries of the twin's full reports."""
import copy
import json

import numpy as np
import pytest

import kyverno_amd as K
from tests.policies import parity_policy_set, pss_policy, restricted_latest, selector_policy

pytestmark = pytest.mark.gpu

N0 = 5000
KPE_E_STATE = 5


@pytest.fixture(scope="module")
def engine():
    return K.Engine(ordinal=0)


def enc(d):
    return json.dumps(d, separators=(",", ":")).encode()


def with_uids(nd, prefix):
    out = []
    for i, line in enumerate(nd.strip(b"\n").split(b"\n")):
        d = json.loads(line)
        d.setdefault("metadata", {})["uid"] = f"{prefix}-{i}"
        out.append(d)
    return out


def name_of(p):
    return p["metadata"]["name"]


def same_rows(got, want):
    assert set(got) == set(want), (sorted(set(got) - set(want))[:8], sorted(set(want) - set(got))[:8])
    for l, row in want.items():
        if row is None:
            assert got[l] is None
        else:
            assert np.array_equal(got[l], row), l


def same_state(a, b):
    assert np.array_equal(a.matrix(), b.matrix())
    na, ca = a.namespace_counts()
    nb, cb = b.namespace_counts()
    assert list(na) == list(nb) and np.array_equal(ca, cb)
    assert a.cli_summary() == b.cli_summary()


class Pair:
    """The scanner under test and its twin, and the policy list both hold."""

    def __init__(self, engine, ndjson, pols):
        self.sc = K.ResidentScanner(engine, ndjson, keyed=True, reports=True)
        self.twin = K.ResidentScanner(engine, ndjson, keyed=True, reports=True)
        self.pols = pols
        self.gone = set()  # logical rows of deleted resources
        ps = K.PolicySet(pols)
        same_rows(self.sc.apply(ps), self.twin.apply(ps))

    def edit(self, new_pols, lazy):
        old = {name_of(p): p for p in self.pols}
        edited = [p for p in new_pols if old.get(name_of(p)) != p]
        removed = [n for n in old if n not in {name_of(p) for p in new_pols}]
        names = {name_of(p) for p in edited}
        full = K.PolicySet(new_pols)
        made = []

        def make():
            made.append(1)
            return K.PolicySet(new_pols)

        sub = K.PolicySet(edited)
        got = self.sc.apply_edit(make if lazy else full, sub, removed)
        assert not made  # nothing needed the whole set yet
        assert self.sc.last_stats["partial"] is True and self.sc.last_stats["columns"] == sub.num_rules
        want = self.twin.apply(full, edited=names)
        same_rows(got, want)
        assert not self.gone & set(got)  # retired rows never come back
        # the edited policies' entries, from the partial evaluation
        rows = sorted(want)[:60]
        part = self.sc.reports(rows, policies="edited")
        whole = self.twin.reports(rows)
        assert not made
        assert set(part) == set(whole)
        for l in rows:
            assert part[l] == [e for e in whole[l] if e["policy"] in names], l
        if names and want:
            assert any(part[l] for l in rows)
        same_state(self.sc, self.twin)
        assert len(made) == (1 if lazy else 0)  # compiled once, by the first reader
        assert self.sc.reports(rows) == whole
        with pytest.raises(K.KpeError) as e:  # the partial evaluation is gone
            self.sc.reports(rows, policies="edited")
        assert e.value.status == KPE_E_STATE
        self.pols = new_pols
        return got


def test_apply_edit_follows_the_twin_through_a_scanners_life(engine):
    P = copy.deepcopy(parity_policy_set())
    pols = ([restricted_latest()] + P[1:6] +
            [selector_policy("ns-prod", kinds=("Pod",), ns_selector={"matchLabels": {"env": "prod"}})])
    docs = with_uids(K.synth_resources(0xE1, N0, mix=K.SYNTH_MIXED), "uid")
    pr = Pair(engine, b"\n".join(enc(d) for d in docs), pols)
    sc, twin = pr.sc, pr.twin

    # 1. an edit under the same name
    p1 = copy.deepcopy(pols)
    p1[4]["spec"]["rules"][0]["validate"]["podSecurity"]["version"] = "v1.0"
    assert len(pr.edit(p1, lazy=True)) > 0

    # 2. update: edited Pods, new resources, deletes
    pods = [i for i, d in enumerate(docs) if d["kind"] == "Pod"]
    ups = []
    for k, i in enumerate(pods[5:5 + 30 * 3:3]):
        d = copy.deepcopy(docs[i])
        d["spec"]["hostNetwork"] = not d["spec"].get("hostNetwork", False)
        d["spec"]["containers"][0].setdefault("securityContext", {})["privileged"] = k % 2 == 1
        ups.append(d)
    new = with_uids(K.synth_resources(0xE2, 9, mix=K.SYNTH_MIXED, first_index=N0), "new")
    dele = [pods[300], pods[301], 1500, 1501]
    nd = b"\n".join(enc(d) for d in ups + new)
    got = sc.update(nd, dele)
    same_rows(got, twin.update(nd, dele))
    assert len(got) > len(dele)
    pr.gone |= set(dele)
    same_state(sc, twin)

    # 3. an edit that adds a policy (over two segments)
    p3 = p1 + [pss_policy("added", "baseline", extra_match={"namespaces": ["ns-00*"]})]
    assert len(sc._segs) == 2
    assert len(pr.edit(p3, lazy=False)) > 0

    # 4. namespace labels: the selector policy starts to match
    nss = sorted({d["metadata"].get("namespace") for d in docs if d["kind"] == "Pod"} - {None})[:3]
    labels = {ns: {"env": "prod"} for ns in nss}
    # ... right after another edit, so the label change meets a partial evaluation
    p4 = copy.deepcopy(p3)
    p4[1]["spec"]["rules"][0]["validate"]["podSecurity"]["version"] = "v1.24"
    old = {name_of(p): p for p in p3}
    sub4 = K.PolicySet([p for p in p4 if old[name_of(p)] != p])
    same_rows(sc.apply_edit(lambda: K.PolicySet(p4), sub4), twin.apply(K.PolicySet(p4), edited={name_of(p4[1])}))
    pr.pols = p4
    got = sc.set_namespace_labels(labels)
    same_rows(got, twin.set_namespace_labels(labels))
    assert len(got) > 0
    same_state(sc, twin)

    # 5. an edit that only removes a policy
    p5 = [p for k, p in enumerate(p4) if k != 2]
    got = pr.edit(p5, lazy=True)
    assert sc.last_stats["columns"] == 0 and len(got) > 0

    # 6. compact, right after an edit
    p6 = copy.deepcopy(p5)
    p6[0]["spec"]["rules"][0]["validate"]["podSecurity"]["level"] = "baseline"
    old = {name_of(p): p for p in p5}
    sub6 = K.PolicySet([p for p in p6 if old[name_of(p)] != p])
    same_rows(sc.apply_edit(lambda: K.PolicySet(p6), sub6), twin.apply(K.PolicySet(p6), edited={name_of(p6[0])}))
    pr.pols = p6
    sc.compact()
    twin.compact()
    assert len(sc._segs) == 1
    same_state(sc, twin)
    assert sc.apply(K.PolicySet(p6)) == {} and twin.apply(K.PolicySet(p6)) == {}

    # 7. an edit on the compacted corpus
    p7 = copy.deepcopy(p6)
    p7[0]["spec"]["rules"][0]["validate"]["podSecurity"]["level"] = "restricted"
    assert len(pr.edit(p7, lazy=True)) > 0


def test_apply_edit_refuses_what_it_cannot_do(engine):
    nd = K.synth_resources(0xE5, 200, mix=K.SYNTH_MIXED)
    pols = [restricted_latest()]
    ps = K.PolicySet(pols)
    sc = K.ResidentScanner(engine, nd)
    with pytest.raises(K.KpeError) as e:  # before the first apply
        sc.apply_edit(ps, ps)
    assert e.value.status == KPE_E_STATE
    fp = K.ResidentScanner(engine, nd, keep="fingerprints")
    fp.apply(ps)
    with pytest.raises(ValueError):
        fp.apply_edit(ps, ps)
    # not keyed: the rows are corpus rows; the twin is a second scanner
    twin = K.ResidentScanner(engine, nd)
    same_rows(sc.apply(ps), twin.apply(ps))
    b = restricted_latest()
    b["spec"]["rules"][0]["validate"]["podSecurity"]["level"] = "baseline"
    psb = K.PolicySet([b])
    got = sc.apply_edit(psb, psb)
    same_rows(got, twin.apply(psb, edited={name_of(b)}))
    assert len(got) > 0
    assert sc.apply(psb) == {}
