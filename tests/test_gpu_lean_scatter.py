"""The scatter form of the compact LEAN evaluation (kpe_lean6_kernel, SC instantiations) on hand-built corpora.

The lane that loaded a list item ORs the item's evidence into the LDS word of the item's owner (the
pod's index in its 64-pod tile, carried by the corpus's owner-tagged columns); a slot past the
tile's item count holds an item of the next tile, whose owner names a pod of this one, and must OR
nothing. Every corpus here is evaluated three ways, and all must be bit-equal to the oracle:

  - the default scatter form, in this process (small corpora: one tile per wave), and in a child
    process at KPE_LEAN6_TPW=4 (four tiles per wave, the shape of the large launches);
  - the gather form over rec12 / cw4, in a child process started with KPE_LEAN6_SHAPE=32;
  - the check-mask evaluation (every versioned check, the wide records).

Under restricted and baseline at `latest`, and baseline v1.0, whose seccomp check reads the
containers' seccomp annotations (the SANN instantiation). Each corpus also takes a cold
evaluation, which rebuilds the tagged columns."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import kyverno_amd as K
from tests.test_gpu_lean_shapes import BATCHED, LEAN6, _sc, poison, pol, stats_of, want_masks
from tests.test_gpu_lean_stream import ctr, ndjson, pod

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = (("restricted", "latest"), ("baseline", "latest"), ("baseline", "v1.0"))
BAD_SC = _sc(privileged=True)
HOSTPATH, EMPTYDIR = {"hostPath": {"path": "/x"}}, {"emptyDir": {}}
GOOD_SYS, BAD_SYS = "kernel.shm_rmid_forced", "kernel.msgmax"
APPARMOR = "container.apparmor.security.beta.kubernetes.io/c0"
SECCOMP_POD = "seccomp.security.alpha.kubernetes.io/pod"
BIG_AT = (0, 63, 64, 127, 128, 191, 199)


def offender(kind, name):
    """A pod whose only finding is in the list `kind`."""
    if kind == "ctr":
        return pod(name, [ctr(0, BAD_SC)])
    if kind == "vol":
        return pod(name, vols=[HOSTPATH])
    if kind == "sys":
        return pod(name, sysctls=[BAD_SYS])
    if kind == "apparmor":
        return pod(name, ann={APPARMOR: "unconfined"})
    return pod(name, ann={SECCOMP_POD: "unconfined"})


def clean_item_pod(kind, name):
    """A clean pod with one harmless item of the list `kind` besides its one clean container."""
    if kind == "vol":
        return pod(name, vols=[EMPTYDIR])
    if kind == "sys":
        return pod(name, sysctls=[GOOD_SYS])
    if kind in ("apparmor", "seccomp"):
        return pod(name, ann={"note": "v"})
    return pod(name)


def boundary_corpus(kind, n):
    """n - 1 clean pods, then one pod that offends in the list `kind`. Every clean pod has one clean
    container and every third one (rows 1, 4, 7, ...: not the first of a tile) one harmless item of
    the list under test, so each full tile's count for that list is 21 (64 for containers): the
    list is scattered, and slot [count] of the last full tile holds the offender's item, whose
    owner, 0, is that tile's clean first pod. `<=` for `<` in the count test fails that pod."""
    pods = [clean_item_pod(kind, f"a{i}") if i % 3 == 1 else pod(f"a{i}") for i in range(n - 1)]
    return pods + [offender(kind, "b")]


def big_pod_corpus():
    """One pod of 200 containers per tile, the offender at position 0, 63, 64, 127, 128, 191 or 199,
    at row 9 of its tile among pods of one clean container: 64-way ORs into one word and the
    batches past the 128 loaded slots."""
    pods = []
    for t, at in enumerate(BIG_AT):
        for i in range(64 if t < len(BIG_AT) - 1 else 12):
            if i == 9:
                pods.append(pod(f"big{t}", [ctr(k, BAD_SC if k == at else None) for k in range(200)]))
            else:
                pods.append(pod(f"p{t}-{i}"))
    return pods


def full_tile_corpus(kind):
    """64 pods of 3 volumes (192 in the tile), 2 sysctls or 2 annotations (128), an offending item
    at each position in turn of every fifth pod; then six clean pods in a tile of their own."""
    pods = []
    for i in range(64):
        bad = i % 5 == 0
        if kind == "vol":
            items = [dict(EMPTYDIR) for _ in range(3)]
            if bad:
                items[(i // 5) % 3] = HOSTPATH
            pods.append(pod(f"v{i}", vols=items))
        elif kind == "sys":
            items = [GOOD_SYS, "net.ipv4.ping_group_range"]
            if bad:
                items[(i // 5) % 2] = BAD_SYS
            pods.append(pod(f"s{i}", sysctls=items))
        else:
            items = [("note-a", "v"), ("note-b", "v")]
            if bad:
                items[(i // 5) % 2] = (APPARMOR, "unconfined") if (i // 10) % 2 else (SECCOMP_POD, "unconfined")
            pods.append(pod(f"n{i}", ann=dict(items)))
    return pods + [pod(f"tail{i}") for i in range(6)]


def empty_corpus():
    """Pods with no item of any list (no containers at all) between neighbours that offend in each
    list in turn, across a tile boundary."""
    kinds = ("ctr", "vol", "sys", "apparmor", "seccomp")
    pods = []
    for i in range(100):
        pods.append(offender(kinds[(i // 2) % len(kinds)], f"o{i}") if i % 2 else pod(f"e{i}", []))
    return pods


def multi_source_corpus():
    """Volumes with several sources (the tagged word's escape: the kernel reads the original mask)
    next to single-source ones and volumes with none."""
    both = {"hostPath": {"path": "/x"}, "emptyDir": {}}
    ok2 = {"emptyDir": {}, "configMap": {"name": "c"}}
    bad2 = {"nfs": {"server": "s", "path": "/"}, "emptyDir": {}}
    sets = ([both], [ok2], [bad2], [EMPTYDIR, both], [ok2, EMPTYDIR], [{}], [EMPTYDIR], [HOSTPATH], [EMPTYDIR, ok2, bad2],
            [{"secret": {"secretName": "s"}}, ok2, {}])
    return [pod(f"m{i}", vols=[dict(v) for v in sets[i % len(sets)]]) for i in range(150)]


CORPORA = {}
for _kind in ("ctr", "vol", "sys", "apparmor", "seccomp"):
    for _n in (65, 129):
        CORPORA[f"boundary-{_kind}-{_n}"] = (lambda k=_kind, n=_n: boundary_corpus(k, n))
CORPORA["big-pod"] = big_pod_corpus
for _kind in ("vol", "sys", "ann"):
    CORPORA[f"full-{_kind}"] = (lambda k=_kind: full_tile_corpus(k))
CORPORA["empty-pods"] = empty_corpus
CORPORA["multi-source"] = multi_source_corpus
# three unequal shards of one launch: in the last partial tile of the last one, the last item of
# every column offends
SHARDS = ("shard-0", "shard-1", "shard-2")
CORPORA["shard-0"] = lambda: boundary_corpus("vol", 70)
CORPORA["shard-1"] = lambda: full_tile_corpus("vol") + empty_corpus()
CORPORA["shard-2"] = lambda: [pod(f"q{i}", vols=[EMPTYDIR] * (i % 3)) for i in range(139)] + [
    pod("last", [ctr(0), ctr(1, BAD_SC)], vols=[EMPTYDIR, HOSTPATH], sysctls=[GOOD_SYS, BAD_SYS],
        ann={"note": "v", APPARMOR: "unconfined"})]
NAMES = list(CORPORA)


def corpus_ndjson(name):
    return ndjson(CORPORA[name]())


def child(out_path):
    """In a process of its own (KPE_LEAN6_SHAPE and KPE_LEAN6_TPW are read when the device is
    opened): every corpus under every level, verdicts only; then the three shards in one launch."""
    eng = K.Engine(ordinal=0)
    sets = [K.PolicySet([pol(*lv)]) for lv in LEVELS]
    out, cs = {}, {}
    for name in NAMES:
        cs[name] = K.Corpus(corpus_ndjson(name), docs=False).upload(eng.device)
        for k, ps in enumerate(sets):
            eng.evaluate_async(ps, cs[name])
            out[f"{name}/{k}"] = eng.fetch(ps, cs[name])[0]
    for k, ps in enumerate(sets):
        batch = [cs[s] for s in SHARDS]
        for c in batch:
            eng.evaluate(ps, c)
            poison(eng, ps, c)
        eng.evaluate_batch_async(ps, batch)
        eng.device.sync()
        for s in SHARDS:
            out[f"batch/{s}/{k}"] = eng.fetch(ps, cs[s])[0]
    out["form"] = np.asarray(lean_form(eng))
    np.savez(out_path, **out)


def lean_form(eng):
    """What the device's last kpe_lean6_kernel launch read: 0 the wide records, 1 rec12 / cw4 (the
    gather form), 2 the owner-tagged columns (the scatter form)."""
    from kyverno_amd._lib import load
    fn = load().kpe_debug_lean_form
    fn.argtypes = [ctypes.c_void_p]
    return fn(eng.device.h)


@pytest.fixture(scope="module")
def engine():
    return K.Engine(ordinal=0)


@pytest.fixture(scope="module")
def refs(oracle):
    """The oracle's verdicts, once per corpus and level."""
    return {name: [oracle.validate([pol(*lv)], corpus_ndjson(name), nthreads=4) for lv in LEVELS] for name in NAMES}


def run_child(tmp_path_factory, tag, **env_add):
    out = str(tmp_path_factory.mktemp(tag) / "out.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("KPE_LEAN6_SHAPE", "KPE_LEAN6_TPW")}
    env.update(env_add, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = f"from tests.test_gpu_lean_scatter import child; child({out!r})"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out)


@pytest.fixture(scope="module")
def gather(tmp_path_factory):
    got = run_child(tmp_path_factory, "gather", KPE_LEAN6_SHAPE="32")
    assert int(got["form"]) == 1, int(got["form"])
    return got


@pytest.fixture(scope="module")
def scatter4(tmp_path_factory):
    got = run_child(tmp_path_factory, "scatter4", KPE_LEAN6_TPW="4")
    assert int(got["form"]) == 2, int(got["form"])
    return got


def test_corpora_offend_where_meant(refs):
    """The references themselves: the clean tiles pass, the offenders fail."""
    for kind in ("ctr", "vol", "sys", "apparmor", "seccomp"):
        for n in (65, 129):
            r, b, b10 = refs[f"boundary-{kind}-{n}"]
            want = b10 if kind == "seccomp" else r if kind in ("ctr", "vol", "sys") else b
            assert (want[:-1, 0] == 1).all() and want[-1, 0] == 2, (kind, n)
    r = refs["big-pod"][0]
    assert [int(i) for i in np.flatnonzero(r[:, 0] == 2)] == [64 * t + 9 for t in range(len(BIG_AT))]
    for kind in ("vol", "sys", "ann"):
        r, b, b10 = refs[f"full-{kind}"]
        bad = (r[:, 0] == 2) | (b10[:, 0] == 2)
        assert [int(i) for i in np.flatnonzero(bad)] == list(range(0, 64, 5)), kind
    r = refs["empty-pods"][0]
    assert (r[0::2, 0] == 1).all()
    assert refs["shard-2"][0][-1, 0] == 2 and refs["shard-2"][1][-1, 0] == 2


@pytest.mark.parametrize("name", NAMES)
def test_three_ways(engine, oracle, refs, gather, scatter4, name):
    """Scatter (here, one tile per wave, warm and cold; and at four tiles per wave), gather
    (KPE_LEAN6_SHAPE=32) and check masks: all the oracle's verdicts."""
    nd = corpus_ndjson(name)
    c = K.Corpus(nd, docs=False).upload(engine.device)
    for k, (level, ver) in enumerate(LEVELS):
        ref = refs[name][k]
        ps = K.PolicySet([pol(level, ver)])
        for cold in (False, True):
            st = stats_of(engine, lambda: engine.evaluate_async(ps, c, cold=cold))
            assert st.scan_kernel == LEAN6 and lean_form(engine) == 2, (st.scan_kernel, lean_form(engine))
            v, _, _ = engine.fetch(ps, c)
            bad = np.argwhere(v != ref)
            assert bad.size == 0, ("scatter", level, ver, cold, len(bad), bad[:5].tolist())
            poison(engine, ps, c)
        for what, got in (("gather", gather), ("scatter, 4 tiles per wave", scatter4)):
            bad = np.argwhere(got[f"{name}/{k}"] != ref)
            assert bad.size == 0, (what, level, ver, len(bad), bad[:5].tolist())
        vm, _, _ = engine.evaluate(ps, c, check_masks=True)
        assert lean_form(engine) == 0  # every check, over the wide records
        assert np.array_equal(vm, ref), ("masks", level, ver, int((vm != ref).sum()))
        assert np.array_equal(engine.cv_masks(ps, c).astype(np.int64), want_masks(oracle, level, ver, nd, vm)), (level, ver)


def test_three_shards_one_launch(engine, refs, gather, scatter4):
    """70, 170 and 140 rows in one launch: the last item of every column offends, in the last
    partial tile of the last shard, and is the last thing before the allocation's slack."""
    cs = [K.Corpus(corpus_ndjson(s), docs=False).upload(engine.device) for s in SHARDS]
    for k, (level, ver) in enumerate(LEVELS):
        ps = K.PolicySet([pol(level, ver)])
        for cold in (False, True):
            for c in cs:
                engine.evaluate(ps, c)
                poison(engine, ps, c)
            st = stats_of(engine, lambda: engine.evaluate_batch_async(ps, cs, cold=cold))
            if not cold:
                assert st.launches == 1 and st.scan_kernel == BATCHED, st.scan_kernel
            assert lean_form(engine) == 2, lean_form(engine)
            engine.device.sync()
            for s, c in zip(SHARDS, cs):
                v, _, _ = engine.fetch(ps, c)
                assert np.array_equal(v, refs[s][k]), (level, ver, cold, s, int((v != refs[s][k]).sum()))
        for s in SHARDS:
            for what, got in (("gather", gather), ("scatter4", scatter4)):
                assert np.array_equal(got[f"batch/{s}/{k}"], refs[s][k]), (what, level, ver, s)
