"""The narrow scatter form of the LEAN evaluation (kpe_lean6_kernel, NW instantiations) on hand-built corpora.

Scatter launches of two or four tiles per wave read a pod as one word of the corpus's pod word
column pw4 (the table slices, class and decode error of the pod word, and the kind id), not as
words x and y of its 12-byte record. The column exists for a corpus of at most 1024 kinds; a launch
with a shard that lacks it reads rec12 for all its shards. Every corpus here is evaluated in three
child processes (the knobs are read when the device is opened), warm and cold (a cold evaluation
rebuilds the columns), under restricted and baseline at `latest` and baseline v1.0 (the SANN
instantiation):

  - KPE_LEAN6_TPW=2 and KPE_LEAN6_TPW=4: the narrow form (kpe_debug_lean_narrow == 1, form 2);
  - KPE_LEAN6_TPW=4 with KPE_LEAN6_SHAPE=64: the same launches over rec12 (narrow == 0, form 2).

All results must be bit-equal to the oracle, and so to each other.

The field corpora sweep every value of every pod-level field the evidence table reads, a decode
error and the three spec classes (Pod, Deployment, CronJob) among unmatched ConfigMaps, at 37, 256,
257 and 1025 rows: a partial tile, exactly one wave at four tiles per wave, one row over, and one
row into a second block. The kind corpora hold 1023 (1024) rows of distinct unmatched kinds and two
Pods, first or last: 1024 kinds, with Pod's kind id the smallest or the largest the word's 10 bits
hold, or 1025 kinds, which keep rec12."""
import copy
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import kyverno_amd as K
from tests.test_gpu_lean_shapes import BATCHED, LEAN6, _sc, poison, pol, stats_of
from tests.test_gpu_lean_stream import GOOD_POD_SC, NEUTRAL_SC, controller, ctr, ndjson, pod

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = (("restricted", "latest"), ("baseline", "latest"), ("baseline", "v1.0"))
BAD_SC = _sc(privileged=True)
FIELD_SIZES = (37, 256, 257, 1025)


def field_rows():
    """One pod per value of each pod-level field with the other fields neutral, a pod that does not
    decode, and controllers of both classes, clean and privileged."""
    rows = []

    def add(name, psc=None, **spec):
        rows.append(pod(name, [ctr(0, dict(NEUTRAL_SC))], psc={**GOOD_POD_SC, **(psc or {})}, **spec))

    add("neutral")
    for key in ("hostNetwork", "hostPID", "hostIPC"):
        for val in (True, False):
            add(key.lower(), **{key: val})
    for val in (True, False):
        add("rnr", {"runAsNonRoot": val})
    add("rnr-unset")
    rows[-1]["spec"]["securityContext"].pop("runAsNonRoot")
    for val in (0, 1000):
        add("rau", {"runAsUser": val})
    for typ in ("RuntimeDefault", "Localhost", "Unconfined", "Bogus"):
        prof = {"type": typ}
        if typ == "Localhost":
            prof["localhostProfile"] = "p.json"
        add("seccomp", {"seccompProfile": prof})
    add("seccomp-unset")
    rows[-1]["spec"]["securityContext"].pop("seccompProfile")
    for typ in ("", "container_t", "container_init_t", "container_kvm_t", "spc_t"):
        for extra in ({}, {"user": "u"}, {"role": "r"}, {"user": "u", "role": "r"}):
            add("sel", {"seLinuxOptions": {"type": typ, **extra}})
    for extra in ({"user": "u"}, {"role": "r"}):  # the sixth type: none given
        add("sel-notype", {"seLinuxOptions": extra})
    for val in (True, False):
        add("whp", {"windowsOptions": {"hostProcess": val}}, hostNetwork=val)
    add("whp-unset", {"windowsOptions": {}})
    for os_name in ("windows", "linux"):
        add("os", os={"name": os_name})
        # a Windows pod is spared the checks that do not apply to it: leave their fields unset
        rows.append(pod("os-bare", [ctr(0, {})], os={"name": os_name}))
    add("decode-error", terminationGracePeriodSeconds="30")
    rows.append(pod("privileged", [ctr(0, BAD_SC)]))
    for kind in ("Deployment", "CronJob"):
        rows.append(controller(kind, "w-clean", [ctr(0)]))
        rows.append(controller(kind, "w-priv", [ctr(0), ctr(1, BAD_SC)]))
    return rows


def configmap(name):
    return {"apiVersion": "v1", "kind": "ConfigMap", "metadata": {"name": name, "namespace": "default"}, "data": {"k": "v"}}


def field_corpus(n):
    """n rows: the field rows in turn (from a start that differs per size), every fifth row a ConfigMap."""
    base, rows = field_rows(), []
    k = n % len(base)
    for i in range(n):
        if i % 5 == 4:
            rows.append(configmap(f"cm-{i}"))
            continue
        o = copy.deepcopy(base[k % len(base)])
        o["metadata"]["name"] += f"-{i}"
        rows.append(o)
        k += 1
    return rows


def kind_corpus(nother, pods_first):
    """`nother` rows of distinct kinds no rule matches and a clean and a privileged Pod. Kind ids
    follow first appearance or the names' order: with the Pods first the other names sort after
    "Pod", with the Pods last before it, so Pod's id is 0 or `nother` either way."""
    pods = [pod("clean"), pod("privileged", [ctr(0, BAD_SC)])]
    pre = "Zk" if pods_first else "Ak"
    other = [{"apiVersion": "example.io/v1", "kind": f"{pre}{i:04d}", "metadata": {"name": f"o{i}", "namespace": "default"},
              "spec": {"x": i}} for i in range(nother)]
    return pods + other if pods_first else other + pods


CORPORA = {f"fields-{n}": (lambda n=n: field_corpus(n)) for n in FIELD_SIZES}
for _nk in (1023, 1024):
    for _first in (True, False):
        CORPORA[f"kinds-{_nk + 1}-{'first' if _first else 'last'}"] = (lambda k=_nk, f=_first: kind_corpus(k, f))
NAMES = list(CORPORA)
NARROW_BATCH = ("fields-1025", "fields-37", "kinds-1024-last")  # every shard has pw4
MIXED_BATCH = ("kinds-1024-first", "kinds-1025-first", "fields-257")  # one shard lacks it: rec12 for all


def has_pw4(name):
    return not name.startswith("kinds-1025")


def corpus_ndjson(name):
    return ndjson(CORPORA[name]())


def debug_int(eng, what):
    """kpe_debug_lean_form: 2 after a scatter launch; kpe_debug_lean_narrow: 1 when it read pw4."""
    from kyverno_amd._lib import load
    fn = getattr(load(), what)
    fn.argtypes = [ctypes.c_void_p]
    fn.restype = ctypes.c_int
    return fn(eng.device.h)


def child(out_path):
    """In a process of its own: every corpus under every level, warm and cold, verdicts only; then
    the two batches, one launch each. Writes the verdicts and, per launch, (form, narrow)."""
    eng = K.Engine(ordinal=0)
    sets = [K.PolicySet([pol(*lv)]) for lv in LEVELS]
    out, cs = {}, {}
    for name in NAMES:
        cs[name] = K.Corpus(corpus_ndjson(name), docs=False).upload(eng.device)
        for k, ps in enumerate(sets):
            for cold in (False, True):
                st = stats_of(eng, lambda: eng.evaluate_async(ps, cs[name], cold=cold))
                key = f"{name}/{k}/{int(cold)}"
                out[key] = eng.fetch(ps, cs[name])[0]
                out["how/" + key] = np.asarray([st.scan_kernel, debug_int(eng, "kpe_debug_lean_form"),
                                                debug_int(eng, "kpe_debug_lean_narrow")])
                poison(eng, ps, cs[name])
    for tag, shards in (("narrow", NARROW_BATCH), ("mixed", MIXED_BATCH)):
        for k, ps in enumerate(sets):
            batch = [cs[s] for s in shards]
            for c in batch:
                eng.evaluate(ps, c)
                poison(eng, ps, c)
            st = stats_of(eng, lambda: eng.evaluate_batch_async(ps, batch))
            eng.device.sync()
            out[f"how/{tag}/{k}"] = np.asarray([st.scan_kernel, debug_int(eng, "kpe_debug_lean_form"),
                                                debug_int(eng, "kpe_debug_lean_narrow"), st.launches])
            for s in shards:
                out[f"{tag}/{s}/{k}"] = eng.fetch(ps, cs[s])[0]
    np.savez(out_path, **out)


@pytest.fixture(scope="module")
def refs(oracle):
    """The oracle's verdicts, once per corpus and level."""
    return {name: [oracle.validate([pol(*lv)], corpus_ndjson(name), nthreads=4) for lv in LEVELS] for name in NAMES}


def run_child(tmp_path_factory, tag, **env_add):
    out = str(tmp_path_factory.mktemp(tag) / "out.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("KPE_LEAN6_SHAPE", "KPE_LEAN6_TPW")}
    env.update(env_add, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = f"from tests.test_gpu_lean_narrow import child; child({out!r})"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out)


@pytest.fixture(scope="module")
def arms(tmp_path_factory):
    """(what, the child's results, is it a narrow arm)"""
    return (("2 tiles per wave", run_child(tmp_path_factory, "tpw2", KPE_LEAN6_TPW="2"), True),
            ("4 tiles per wave", run_child(tmp_path_factory, "tpw4", KPE_LEAN6_TPW="4"), True),
            ("rec12 arm", run_child(tmp_path_factory, "rec12", KPE_LEAN6_TPW="4", KPE_LEAN6_SHAPE="64"), False))


def test_corpora_hold_what_is_meant(refs):
    """The references themselves."""
    base = field_rows()
    assert max(FIELD_SIZES) - max(FIELD_SIZES) // 5 >= len(base)  # the largest corpus holds every field row
    for n in FIELD_SIZES:
        r, b, b10 = refs[f"fields-{n}"]
        assert r.shape[0] == n and (r[4::5] == 0).all()  # the ConfigMaps: no rule matches
    r = refs["fields-1025"][0]
    assert {int(x) for x in np.unique(r[:, 0])} >= {0, 1, 2, 4}  # unmatched, pass, fail, error (the decode error)
    for nk in (1024, 1025):
        for first in (True, False):
            for k in range(len(LEVELS)):
                v = refs[f"kinds-{nk}-{'first' if first else 'last'}"][k]
                pods = v[:2] if first else v[-2:]
                rest = v[2:] if first else v[:-2]
                assert pods.tolist() == [[1, 0, 0], [2, 0, 0]] and (rest == 0).all(), (nk, first, k)


@pytest.mark.parametrize("name", NAMES)
def test_narrow_equals_rec12_equals_oracle(refs, arms, name):
    """Each corpus alone, warm and cold: the narrow form where the corpus has pw4 and the knob is
    clear, always a scatter launch, always the oracle's verdicts."""
    for what, got, narrow_arm in arms:
        for k, (level, ver) in enumerate(LEVELS):
            for cold in (0, 1):
                key = f"{name}/{k}/{cold}"
                kind, form, narrow = (int(x) for x in got["how/" + key])
                assert kind == LEAN6 and form == 2, (what, key, kind, form)
                assert narrow == int(narrow_arm and has_pw4(name)), (what, key, narrow)
                bad = np.argwhere(got[key] != refs[name][k])
                assert bad.size == 0, (what, level, ver, cold, len(bad), bad[:5].tolist())


def test_batches(refs, arms):
    """Three shards in one launch: all with pw4 (narrow), and with one of 1025 kinds among them
    (rec12 for all three)."""
    for what, got, narrow_arm in arms:
        for tag, shards in (("narrow", NARROW_BATCH), ("mixed", MIXED_BATCH)):
            for k, (level, ver) in enumerate(LEVELS):
                kind, form, narrow, launches = (int(x) for x in got[f"how/{tag}/{k}"])
                assert launches == 1 and kind == BATCHED and form == 2, (what, tag, k, launches, kind, form)
                assert narrow == int(narrow_arm and tag == "narrow"), (what, tag, k, narrow)
                for s in shards:
                    v = got[f"{tag}/{s}/{k}"]
                    assert np.array_equal(v, refs[s][k]), (what, tag, level, ver, s, int((v != refs[s][k]).sum()))
