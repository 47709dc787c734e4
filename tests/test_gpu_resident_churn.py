"""ResidentScanner(keyed=True) under resource churn: `update` (upserts and deletes between policy
changes), `apply` over the segments, `compact`, `reports`, `matrix`, for keep="matrix" and
keep="fingerprints". After every step the scanner's matrix by logical row equals the oracle's over
the current resource list, and the returned set is exactly the rows whose oracle rows differ between
the two states (plus the edited policy's FAIL / ERROR / SKIP cells at `apply`, and None for deletes).
A label-only edit changes a resource's hash and nothing in its report: it is rescanned and must not
come back."""
import copy
import json

import numpy as np
import pytest

import kyverno_amd as K
from kyverno_amd.scan import _key
from tests.policies import parity_policy_set, restricted_latest

pytestmark = pytest.mark.gpu

FAIL, ERROR, SKIP = 2, 4, 5
N0 = 3000


@pytest.fixture(scope="module")
def engine():
    return K.Engine(ordinal=0)


def with_uids(nd, prefix):
    out = []
    for i, line in enumerate(nd.strip(b"\n").split(b"\n")):
        d = json.loads(line)
        d.setdefault("metadata", {})["uid"] = f"{prefix}-{i}"
        out.append(d)
    return out


def enc(d):
    return json.dumps(d, separators=(",", ":")).encode()


def policy_sets():
    P = copy.deepcopy(parity_policy_set())
    p1 = [restricted_latest()] + P[1:6]
    p2 = copy.deepcopy(p1)
    p2[4]["spec"]["rules"][0]["validate"]["podSecurity"]["version"] = "v1.0"  # one policy edited, under its name
    return p1, p2, {p2[4]["metadata"]["name"]}


class World:
    """The resources by logical row (None: deleted) and the oracle's matrix of a state."""

    def __init__(self, oracle, docs):
        self.oracle = oracle
        self.cur = list(docs)

    def live(self):
        return [i for i, d in enumerate(self.cur) if d is not None]

    def ndjson(self):
        return b"\n".join(enc(self.cur[i]) for i in self.live())

    def matrix(self, pols, R):
        out = np.zeros((len(self.cur), R), dtype=np.uint8)
        live = self.live()
        if live:
            out[live] = self.oracle.validate(pols, self.ndjson(), nthreads=8)
        return out


def pad(m, n):
    return np.vstack([m, np.zeros((n - m.shape[0], m.shape[1]), dtype=np.uint8)]) if m.shape[0] < n else m


def check_update(got, before, after, deleted):
    """Exactly the rows whose oracle rows differ, and None for every deleted resource."""
    before = pad(before, after.shape[0])
    want = set(np.flatnonzero((before != after).any(axis=1)).tolist()) - set(deleted) | set(deleted)
    assert set(got) == want, (sorted(set(got) - want)[:8], sorted(want - set(got))[:8])
    for l, row in got.items():
        if l in deleted:
            assert row is None
        else:
            assert np.array_equal(row, after[l])


def check_reports(engine, sc, world, pols, ps, rows):
    """reports(rows) against a fresh scanner over the current list."""
    live = world.live()
    pos = {l: k for k, l in enumerate(live)}
    got = sc.reports(rows)
    assert set(got) == set(int(r) for r in rows)
    fresh = K.ResidentScanner(engine, world.ndjson(), reports=True)
    fresh.apply(ps)
    alive = [int(r) for r in rows if world.cur[int(r)] is not None]
    want = fresh.reports([pos[l] for l in alive])
    for l in alive:
        assert got[l] == want[pos[l]], l
    for r in rows:
        if world.cur[int(r)] is None:
            assert got[int(r)] == []


@pytest.mark.parametrize("keep", ["matrix", "fingerprints"])
def test_churn_scenario(engine, oracle, keep):
    pols1, pols2, edited = policy_sets()
    ps1, ps2 = K.PolicySet(pols1), K.PolicySet(pols2)
    R = ps1.num_rules
    assert ps2.rule_names == ps1.rule_names
    docs = with_uids(K.synth_resources(0xE1, N0, mix=K.SYNTH_MIXED), "uid")
    world = World(oracle, docs)
    sc = K.ResidentScanner(engine, world.ndjson(), keep=keep, reports=True, keyed=True)
    assert len(sc.resource_hashes) == N0

    # 1. apply(P1): every row with a response
    m1 = world.matrix(pols1, R)
    got = sc.apply(ps1)
    assert set(got) == set(np.flatnonzero((m1 != 0).any(axis=1)).tolist())
    assert all(np.array_equal(got[l], m1[l]) for l in got)
    assert np.array_equal(sc.matrix(), m1)

    # 2. update: 37 Pods edited (odd ones in a way that can flip a verdict, even ones a label only), 7 offered
    # unchanged, 11 new resources, 5 deletes (three by key, two by logical row)
    pods = [i for i, d in enumerate(docs) if d["kind"] == "Pod"]
    edit = pods[5:5 + 37 * 3:3]
    assert len(edit) == 37
    label_only = set()
    ups = []
    for k, i in enumerate(edit):
        d = copy.deepcopy(world.cur[i])
        if k % 2 == 0:
            d["metadata"].setdefault("labels", {})["churn"] = f"e{k}"
            label_only.add(i)
        else:
            d["spec"]["hostNetwork"] = not d["spec"].get("hostNetwork", False)
            d["spec"]["containers"][0].setdefault("securityContext", {})["privileged"] = k % 4 == 1
        world.cur[i] = d
        ups.append(d)
    same = [world.cur[i] for i in pods[200:207]]
    new = with_uids(K.synth_resources(0xE2, 11, mix=K.SYNTH_MIXED, first_index=N0), "new")
    dele = [pods[300], pods[301], 1500, 1501, 1502]
    assert not set(dele) & set(edit)
    deletes = [_key(enc(world.cur[dele[0]]), 0), _key(enc(world.cur[dele[1]]), 0), _key(enc(world.cur[dele[2]]), 0), dele[3],
               dele[4]]
    for i in dele:
        world.cur[i] = None
    world.cur.extend(new)
    got = sc.update(b"\n".join(enc(d) for d in ups + same + new), deletes)
    m2 = world.matrix(pols1, R)
    assert sc.last_stats["skipped"] == 7 and sc.last_stats["rescanned"] == 37 + 11 and sc.last_stats["deleted"] == 5
    check_update(got, m1, m2, set(dele))
    assert np.array_equal(sc.matrix(), m2)
    assert not label_only & set(got)  # rescanned, report unchanged: must not come back
    assert (set(edit) - label_only) & set(got)  # and some edits did flip a verdict
    assert any(l >= N0 for l in got)  # new resources with a response, at appended logical rows
    check_reports(engine, sc, world, pols1, ps1, sorted(got))
    if keep == "fingerprints":
        rows, fps = sc.fingerprints()
        assert rows.tolist() == world.live()
        assert np.array_equal(fps != 0, (m2[world.live()] != 0).any(axis=1))

    # 3. apply(P2), one policy edited: the twin over the two logical matrices
    m3 = world.matrix(pols2, R)
    always = np.array([(K.SEL(FAIL) | K.SEL(ERROR) | K.SEL(SKIP)) if n.split("/", 1)[0] in edited else 0
                       for n in ps2.rule_names], dtype=np.uint8)
    want_rows, want_vr, _ = K.changed_rows(m2, m3, np.arange(R, dtype=np.int32), always)
    got = sc.apply(ps2, edited=edited)
    assert sorted(got) == want_rows.tolist() and len(got) > 0
    assert all(np.array_equal(got[int(l)], want_vr[k]) for k, l in enumerate(want_rows))
    assert np.array_equal(sc.matrix(), m3)
    assert sc.last_stats["segments"] == 2
    check_reports(engine, sc, world, pols2, ps2, sorted(got)[:40])
    assert sc.apply(ps2) == {}

    # 4. a second update: a row of the first delta segment edited, one of them deleted, one old row edited
    l_new = N0 + 3
    d = copy.deepcopy(world.cur[l_new])
    d["metadata"].setdefault("labels", {})["churn"] = "again"
    if d["kind"] == "Pod":
        d["spec"]["hostPID"] = True
    world.cur[l_new] = d
    l_old = edit[1]  # already replaced once: it lives in the delta segment too
    d2 = copy.deepcopy(world.cur[l_old])
    d2["spec"]["hostNetwork"] = not d2["spec"].get("hostNetwork", False)
    world.cur[l_old] = d2
    l_first = pods[10]
    d3 = copy.deepcopy(world.cur[l_first])
    d3["spec"]["hostIPC"] = True
    world.cur[l_first] = d3
    world.cur[N0 + 5] = None
    got = sc.update(b"\n".join(enc(x) for x in (d, d2, d3)), [N0 + 5])
    m4 = world.matrix(pols2, R)
    check_update(got, m3, m4, {N0 + 5})
    assert np.array_equal(sc.matrix(), m4)
    assert sc.last_stats["segments"] == 3 and sc.last_stats["skipped"] == 0
    check_reports(engine, sc, world, pols2, ps2, sorted(got))

    # 5. compact: one segment, the same matrix, the same logical rows
    sc.compact()
    assert len(sc._segs) == 1 and sc.corpus.n == len(world.live())
    assert np.array_equal(sc.matrix(), m4)
    assert sc.apply(ps2) == {}  # the recompute reports nothing
    check_reports(engine, sc, world, pols2, ps2, [l_old, l_first, N0 + 5, 0])

    # 6. apply(P1) again
    m6 = world.matrix(pols1, R)
    always = np.array([(K.SEL(FAIL) | K.SEL(ERROR) | K.SEL(SKIP)) if n.split("/", 1)[0] in edited else 0
                       for n in ps1.rule_names], dtype=np.uint8)
    want_rows, want_vr, _ = K.changed_rows(m4, m6, np.arange(R, dtype=np.int32), always)
    got = sc.apply(ps1, edited=edited)
    assert sorted(got) == want_rows.tolist() and len(got) > 0
    assert all(np.array_equal(got[int(l)], want_vr[k]) for k, l in enumerate(want_rows))
    assert np.array_equal(sc.matrix(), m6)


@pytest.mark.parametrize("keep", ["matrix", "fingerprints"])
def test_update_before_the_first_apply_and_automatic_compaction(engine, oracle, keep):
    pols1, _, _ = policy_sets()
    ps1 = K.PolicySet(pols1)
    docs = with_uids(K.synth_resources(0xE3, 200, mix=K.SYNTH_MIXED), "uid")
    world = World(oracle, docs)
    sc = K.ResidentScanner(engine, world.ndjson(), keep=keep, keyed=True, max_segments=2, max_retired=0.25)
    # nothing applied yet: the corpus is restructured, nothing is reported
    d = copy.deepcopy(world.cur[7])
    d["metadata"].setdefault("labels", {})["x"] = "y"
    world.cur[7] = d
    world.cur[9] = None
    assert sc.update(enc(d), [9]) == {}
    assert sc.last_stats["segments"] == 2 and "compacted" not in sc.last_stats
    m = world.matrix(pols1, ps1.num_rules)
    got = sc.apply(ps1)
    assert set(got) == set(np.flatnonzero((m != 0).any(axis=1)).tolist())
    assert np.array_equal(sc.matrix(), m)
    # a third segment: past max_segments, update compacts
    d = copy.deepcopy(world.cur[8])
    d["metadata"].setdefault("labels", {})["x"] = "z"
    world.cur[8] = d
    assert sc.update(enc(d)) == {}  # a label only
    assert sc.last_stats.get("compacted")
    assert len(sc._segs) == 1 and np.array_equal(sc.matrix(), world.matrix(pols1, ps1.num_rules))
    assert sc.apply(ps1) == {}
    # more than a quarter of the physical rows retired: compaction again
    live = world.live()
    gone = live[:60]
    for i in gone:
        world.cur[i] = None
    got = sc.update(b"", gone)
    assert set(got) == set(gone) and all(v is None for v in got.values())
    assert sc.last_stats.get("compacted") and sc.corpus.n == len(world.live())
    assert np.array_equal(sc.matrix(), world.matrix(pols1, ps1.num_rules))
    assert sc.apply(ps1) == {}
    # a scanner that is not keyed refuses
    with pytest.raises(K.KpeError):
        K.ResidentScanner(engine, world.ndjson()).update(b"")
