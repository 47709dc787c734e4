"""The group form of the LEAN evaluation's narrow scatter (kpe_lean6_kernel, GR instantiations) on
hand-built corpora.

A narrow launch of four tiles per wave streams each wave's volumes, sysctls and annotations as one
256-pod group: the item words carry the pod's tile within the group, a slot counts while its index
is below the group's item count, and every pod's evidence is one of 256 interleaved words. Every
corpus here is evaluated in two child processes (the knobs are read when the device is opened):

  - KPE_LEAN6_TPW=4: the group form (kpe_debug_lean_group == 1, narrow 1, form 2);
  - KPE_LEAN6_TPW=4 with KPE_LEAN6_SHAPE=128: the per-tile form over the same columns (group == 0).

All verdicts must equal the oracle's, and so each other's, under restricted:latest (R = 3) and under
a set of five rules with three version classes (R = 5: rows leave through the byte path).

Corpora of 193, 256, 257 and 1025 rows: three tiles of a group and a partial fourth, exactly one
group, one row into a second group, and one row into a second block. `lists-<kind>-<n>`: clean
groups with few items (every third pod none at all) alternate with groups whose tiles begin with 24
pods offending in that list (kind `all`: in every list), so the slots past a clean group's count
hold the next group's offending items; in the corpora of one group the tiles alternate instead.
`long-257`: a group with more items than the sets loaded up front (two pods of 250 volumes, the
most a pod may hold being 255, one of 100 sysctls and one of 200 annotations, the offending item
last each time, past the up-front slots), and volumes with several sources, allowed and not.
The mixed batch holds a shard of 1025 kinds, which has no pod word column: the launch is not
narrow and keeps the per-tile form for all its shards."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kyverno_amd as K
from tests.policies import pss_policy
from tests.test_gpu_lean_narrow import debug_int, kind_corpus
from tests.test_gpu_lean_shapes import BATCHED, LEAN6, poison, pol, stats_of
from tests.test_gpu_lean_stream import ndjson, pod

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_AUTOGEN = {"pod-policies.kyverno.io/autogen-controllers": "none"}
APPARMOR = "container.apparmor.security.beta.kubernetes.io/c0"
PASS, FAIL = 1, 2


def one_rule(name, level, ver):
    p = pss_policy(name, level, ver)
    p["metadata"]["annotations"] = dict(NO_AUTOGEN)
    return p


def policy_sets():
    """R = 3 (the Pod rule and its two autogen rules) and R = 5 (two single rules of other version classes more)."""
    r3 = [pol("restricted", "latest")]
    return (r3, r3 + [one_rule("b-latest", "baseline", "latest"), one_rule("r-1-24", "restricted", "v1.24")])


def clean(i):
    return pod(f"p{i}", vols=[{"emptyDir": {}}] * (i % 3), sysctls=["kernel.shm_rmid_forced"] * (i % 5 == 0 and i % 3 != 0),
               ann={"note": "v"} if i % 4 == 0 and i % 3 else None)


def bad(kind, i):
    vols = [{"emptyDir": {}}, {"hostPath": {"path": "/x"}}] if kind in ("vol", "all") else ()
    sysctls = ["kernel.msgmax"] if kind in ("sys", "all") else ()
    ann = {APPARMOR: "unconfined"} if kind in ("ann", "all") else None
    return pod(f"bad{i}", vols=vols, sysctls=sysctls, ann=ann)


def is_bad(n, i):
    hot = (i // 256) % 2 == 1 if n > 256 else (i // 64) % 2 == 1
    return hot and i % 64 < 24


def lists_corpus(kind, n):
    return [bad(kind, i) if is_bad(n, i) else clean(i) for i in range(n)]


LONG = {10: "v-clean", 11: "v-bad", 20: "s-bad", 30: "a-bad", 40: "multi-bad", 41: "multi-clean"}


def long_corpus():
    rows = [clean(i) for i in range(257)]
    empty, secret = {"emptyDir": {}}, {"secret": {"secretName": "s"}}
    rows[10] = pod("v-clean", vols=[empty] * 250)
    rows[11] = pod("v-bad", vols=[secret] * 249 + [{"hostPath": {"path": "/x"}}])
    rows[20] = pod("s-bad", sysctls=["kernel.shm_rmid_forced"] * 99 + ["kernel.msgmax"])
    rows[30] = pod("a-bad", ann={**{f"note{k}": "v" for k in range(199)}, APPARMOR: "unconfined"})
    rows[40] = pod("multi-bad", vols=[{"emptyDir": {}, "hostPath": {"path": "/x"}}])
    rows[41] = pod("multi-clean", vols=[{"emptyDir": {}, "secret": {"secretName": "s"}}])
    rows[256] = bad("all", 256)
    return rows


CORPORA = {"lists-all-193": lambda: lists_corpus("all", 193), "lists-all-256": lambda: lists_corpus("all", 256),
           "long-257": long_corpus}
for _kind in ("vol", "sys", "ann"):
    for _n in (257, 1025):
        CORPORA[f"lists-{_kind}-{_n}"] = (lambda k=_kind, n=_n: lists_corpus(k, n))
CORPORA["kinds-1025"] = lambda: kind_corpus(1024, True)  # no pod word column: never narrow, never the group form
NAMES = list(CORPORA)
GROUP_BATCH = ("lists-vol-1025", "lists-all-193", "long-257")
MIXED_BATCH = ("lists-ann-257", "kinds-1025", "lists-sys-1025")


def corpus_ndjson(name):
    return ndjson(CORPORA[name]())


def how(eng, st):
    return np.asarray([st.scan_kernel, st.launches] +
                      [debug_int(eng, f"kpe_debug_lean_{w}") for w in ("form", "narrow", "group")])


def child(out_path):
    """In a process of its own: every corpus under both policy sets, then the two batches, one
    launch each. Writes the verdicts and, per launch, (kernel, launches, form, narrow, group)."""
    eng = K.Engine(ordinal=0)
    sets = [K.PolicySet(ps) for ps in policy_sets()]
    out, cs = {}, {}
    for name in NAMES:
        cs[name] = K.Corpus(corpus_ndjson(name), docs=False).upload(eng.device)
        for k, ps in enumerate(sets):
            st = stats_of(eng, lambda: eng.evaluate_async(ps, cs[name]))
            out[f"{name}/{k}"] = eng.fetch(ps, cs[name])[0]
            out[f"how/{name}/{k}"] = how(eng, st)
            poison(eng, ps, cs[name])
    for tag, shards in (("group", GROUP_BATCH), ("mixed", MIXED_BATCH)):
        for k, ps in enumerate(sets):
            batch = [cs[s] for s in shards]
            for c in batch:
                eng.evaluate(ps, c)
                poison(eng, ps, c)
            st = stats_of(eng, lambda: eng.evaluate_batch_async(ps, batch))
            eng.device.sync()
            out[f"how/{tag}/{k}"] = how(eng, st)
            for s in shards:
                out[f"{tag}/{s}/{k}"] = eng.fetch(ps, cs[s])[0]
    np.savez(out_path, **out)


@pytest.fixture(scope="module")
def refs(oracle):
    """The oracle's verdicts, once per corpus and policy set."""
    return {name: [oracle.validate(ps, corpus_ndjson(name), nthreads=4) for ps in policy_sets()] for name in NAMES}


def run_child(tmp_path_factory, tag, **env_add):
    out = str(tmp_path_factory.mktemp(tag) / "out.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("KPE_LEAN6_SHAPE", "KPE_LEAN6_TPW")}
    env.update(env_add, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = f"from tests.test_gpu_lean_group import child; child({out!r})"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out)


@pytest.fixture(scope="module")
def arms(tmp_path_factory):
    """(what, the child's results, is it the group arm)"""
    return (("group form", run_child(tmp_path_factory, "group", KPE_LEAN6_TPW="4"), True),
            ("per-tile form", run_child(tmp_path_factory, "tile", KPE_LEAN6_TPW="4", KPE_LEAN6_SHAPE="128"), False))


def test_corpora_hold_what_is_meant(refs):
    """The references themselves: the rule of the Pod kind fails exactly the offending pods."""
    r3, r5 = policy_sets()
    assert len(r3) == 1 and len(r5) == 3
    for name in NAMES:
        v3, v5 = refs[name]
        assert v3.shape[1] == 3 and v5.shape[1] == 5, (name, v3.shape, v5.shape)
        if name.startswith("lists-"):
            n = v3.shape[0]
            want = np.asarray([FAIL if is_bad(n, i) else PASS for i in range(n)])
            assert np.array_equal(v3[:, 0], want), name
            assert (want == FAIL).any() and want[0] == PASS
    v3, v5 = refs["long-257"]
    for i, what in LONG.items():
        assert v3[i, 0] == (FAIL if what.endswith("bad") else PASS), (i, what, v3[i].tolist())
    assert v3[256, 0] == FAIL and v5[256, 3] == FAIL  # the baseline rule too: hostPath, sysctl, AppArmor
    assert refs["kinds-1025"][0][:2].tolist() == [[1, 0, 0], [2, 0, 0]]


@pytest.mark.parametrize("name", NAMES)
def test_group_equals_per_tile_equals_oracle(refs, arms, name):
    """Each corpus alone: the group form where the corpus has the pod word column and the knob is
    clear, always a scatter launch, always the oracle's verdicts."""
    narrow_corpus = name != "kinds-1025"
    for what, got, group_arm in arms:
        for k in range(2):
            key = f"{name}/{k}"
            kind, launches, form, narrow, group = (int(x) for x in got["how/" + key])
            assert kind == LEAN6 and launches == 1 and form == 2, (what, key, kind, launches, form)
            assert narrow == int(narrow_corpus) and group == int(group_arm and narrow_corpus), (what, key, narrow, group)
            bad_cells = np.argwhere(got[key] != refs[name][k])
            assert bad_cells.size == 0, (what, key, len(bad_cells), bad_cells[:5].tolist())
    for k in range(2):
        assert np.array_equal(arms[0][1][f"{name}/{k}"], arms[1][1][f"{name}/{k}"]), (name, k)


def test_batches(refs, arms):
    """Three shards in one launch: all with the pod word column (the group form), and with a shard
    of 1025 kinds among them (the per-tile form over rec12 for all three)."""
    for what, got, group_arm in arms:
        for tag, shards in (("group", GROUP_BATCH), ("mixed", MIXED_BATCH)):
            for k in range(2):
                kind, launches, form, narrow, group = (int(x) for x in got[f"how/{tag}/{k}"])
                assert launches == 1 and kind == BATCHED and form == 2, (what, tag, k, launches, kind, form)
                assert narrow == int(tag == "group") and group == int(group_arm and tag == "group"), (what, tag, k, narrow, group)
                for s in shards:
                    v = got[f"{tag}/{s}/{k}"]
                    assert np.array_equal(v, refs[s][k]), (what, tag, k, s, int((v != refs[s][k]).sum()))
