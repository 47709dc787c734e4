"""The LEAN evaluation over the corpus's compact columns (12-byte pod records, one word per
container: kernels_abi.h KPE_L6C_*, built by kpe_lean_pack_kernel) on hand-built corpora.

Every corpus is evaluated three ways: verdicts only over the compact columns (this process), verdicts
only over the wide records (KPE_LEAN6_SHAPE=16, read when the device is opened: a child process),
and with check masks (the form that decides every versioned check from the wide records). All
three are held to the oracle, compact and wide to each other bit for bit, and the check masks to
the oracle's failing checks. The corpora: the tile and block edges at 4 tiles per wave, containers
none of whose used state bits is set (they must count as present), 2,048 distinct capability sets,
pods of 0, 4, 5 and 9 containers, a tile of more than 128 containers, the column's last container,
controller kinds and a kind outside the kind table, three unequal shards in one launch, and a
cold evaluation (which rebuilds the compact columns)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kyverno_amd as K
from tests.test_gpu_lean_shapes import BATCHED, LEAN6, _sc, poison, pol, stats_of, want_masks
from tests.test_gpu_lean_stream import controller, ctr, ndjson, pod, rows_ndjson

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
BATCH = ("rows_65", "capsets", "rows_257")  # 65, 2100 and 257 rows in one launch
LEVELS = (("restricted", "latest"), ("baseline", "latest"))
BAD = _sc(privileged=True)
# a container none of whose used state bits is set, every field spelled out
CLEAR = {"privileged": False, "allowPrivilegeEscalation": False, "runAsNonRoot": True, "runAsUser": 1000,
         "seccompProfile": {"type": "RuntimeDefault"}, "procMount": "Default",
         "seLinuxOptions": {"type": "container_t"}, "windowsOptions": {"hostProcess": False}}
CAPS = ("NET_BIND_SERVICE", "CHOWN", "KILL", "SETUID", "SETGID", "FOWNER", "MKNOD", "SYS_ADMIN", "NET_ADMIN", "SYS_TIME",
        "NET_RAW")


def clear_ndjson():
    """Containers with no used state bit, whose only finding (if any) is their capability set: alone
    in the corpus's first pod, as a pod's only container between offending neighbours, and beside
    a container that has state bits. Read as an empty slot, the capability finding is lost."""
    drop_all, no_drop = {"drop": ["ALL"]}, {"add": ["SYS_ADMIN"]}
    pods = [pod("alone", [ctr(0, {**CLEAR, "capabilities": no_drop})])]
    for i, caps in enumerate((drop_all, no_drop, {"drop": ["ALL"], "add": ["NET_ADMIN"]}, {"drop": ["KILL"]})):
        pods.append(pod(f"l{i}", [ctr(0, BAD)]))
        pods.append(pod(f"only{i}", [ctr(0, {**CLEAR, "capabilities": caps})]))
        pods.append(pod(f"r{i}", [ctr(0, BAD)]))
        pods.append(pod(f"pair{i}", [ctr(0, _sc(allowPrivilegeEscalation=None)), ctr(1, {**CLEAR, "capabilities": caps})]))
        pods.append(pod(f"good{i}", [ctr(0, {**CLEAR, "capabilities": drop_all})]))
    return ndjson(pods)


def capsets_ndjson():
    """2,100 pods of one container: pod i adds the capabilities of the bits of i % 2048 and drops ALL,
    so the corpus has 2,048 distinct capability sets (the dictionary's limit: ids 0 to 2047). The
    first set (nothing added) passes restricted, the last (all eleven) fails it."""
    pods = []
    for i in range(2100):
        add = [c for b, c in enumerate(CAPS) if (i % 2048) >> b & 1]
        caps = {"drop": ["ALL"], **({"add": add} if add else {})}
        pods.append(pod(f"p{i}", [ctr(0, {**CLEAR, "capabilities": caps})]))
    return ndjson(pods)


def counts_ndjson():
    """Pods of 0, 4, 5 and 9 containers, the offending one at each position or absent, between
    offending neighbours: four clamped reads, and the loop over a pod's containers past them."""
    pods = []
    for nc in (0, 4, 5, 9):
        for at in [None] + list(range(nc)):
            pods.append(pod(f"l{len(pods)}", [ctr(0, BAD)]))
            pods.append(pod(f"t{len(pods)}", [ctr(k, BAD if k == at else None) for k in range(nc)]))
            pods.append(pod(f"r{len(pods)}", [ctr(0, BAD)]))
    return ndjson(pods)


def overflow_ndjson():
    """A tile of 64 pods x 3 containers (192: the stage holds 128, the rest is loaded again from the
    column), an offending container at each position of every fifth pod; then a partial tile whose
    last pod's last container, the column's last word, offends."""
    pods = []
    for i in range(64):
        at = i % 3 if i % 5 == 0 else None
        pods.append(pod(f"o{i}", [ctr(k, BAD if k == at else None) for k in range(3)]))
    pods.append(pod("tail0", [ctr(0)]))
    pods.append(pod("tail1", [ctr(k, BAD if k == 4 else None) for k in range(5)]))
    return ndjson(pods)


def end_ndjson():
    """Three pods; the last has one container, offending: the clamped reads of the last pod reach
    past the column's end, which must read as empty slots."""
    return ndjson([pod("a", [ctr(0)]), pod("b", [ctr(0), ctr(1)]), pod("c", [ctr(0, BAD)])])


def kinds_ndjson():
    """Controller kinds (their rules are the autogen ones) with and without an offending container, a
    kind no rule names, and pods between them."""
    pods = []
    for kind in ("Deployment", "DaemonSet", "StatefulSet", "CronJob"):
        for bad in (False, True):
            pods.append(pod(f"l{len(pods)}", [ctr(0, BAD)]))
            pods.append(controller(kind, f"w{len(pods)}", [ctr(0, BAD if bad else None)]))
    pods.append({"apiVersion": "v1", "kind": "ConfigMap", "metadata": {"name": "cm", "namespace": "default"},
                 "data": {"k": "v"}})
    pods.append(pod("last", [ctr(0)]))
    return ndjson(pods)


CORPORA = {**{f"rows_{n}": (lambda n=n: rows_ndjson(n)) for n in ROW_COUNTS}, "clear": clear_ndjson,
           "capsets": capsets_ndjson, "counts": counts_ndjson, "overflow": overflow_ndjson, "end": end_ndjson,
           "kinds": kinds_ndjson}


def run_all(eng):
    """Every corpus under both levels: verdicts only (v), after a cold evaluation (cold), with
    check masks (m, cv), the launch's algorithmic bytes (bytes); then the batch (b)."""
    out = {}
    sets = {lv: K.PolicySet([pol(*lv)]) for lv in LEVELS}
    cs = {}
    for name, build in CORPORA.items():
        cs[name] = c = K.Corpus(build(), docs=False).upload(eng.device)
        for lv in LEVELS:
            ps, key = sets[lv], f"{name}_{lv[0]}"
            st = stats_of(eng, lambda: eng.evaluate_async(ps, c))
            assert st.launches == 1 and st.scan_kernel == LEAN6, (name, st.scan_kernel)
            out[f"bytes_{key}"] = np.float64(st.scan_bytes)
            out[f"v_{key}"] = eng.fetch(ps, c)[0]
            poison(eng, ps, c)
            eng.evaluate_async(ps, c, cold=True)
            out[f"cold_{key}"] = eng.fetch(ps, c)[0]
            poison(eng, ps, c)
            out[f"m_{key}"] = eng.evaluate(ps, c, check_masks=True)[0]
            out[f"cv_{key}"] = eng.cv_masks(ps, c).astype(np.int64)
    ps = sets[LEVELS[0]]
    batch = [cs[name] for name in BATCH]
    for c in batch:
        eng.evaluate(ps, c)
        poison(eng, ps, c)
    st = stats_of(eng, lambda: eng.evaluate_batch_async(ps, batch))
    assert st.launches == 1 and st.scan_kernel == BATCHED, st.scan_kernel
    eng.device.sync()
    for name, c in zip(BATCH, batch):
        out[f"b_{name}"] = eng.fetch(ps, c)[0]
    return out


def wide_child(out_path):
    assert os.environ["KPE_LEAN6_SHAPE"] == "16"
    np.savez(out_path, **run_all(K.Engine(ordinal=0)))


@pytest.fixture(scope="module")
def compact():
    assert "KPE_LEAN6_SHAPE" not in os.environ
    return run_all(K.Engine(ordinal=0))


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    """The same in a process of its own, its verdict-only launches over the wide records."""
    out = str(tmp_path_factory.mktemp("wide") / "wide.npz")
    env = dict(os.environ, KPE_LEAN6_SHAPE="16", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = f"from tests.test_gpu_lean_compact import wide_child; wide_child({out!r})"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return dict(np.load(out))


@pytest.fixture(scope="module")
def refs(oracle):
    out = {}
    for name, build in CORPORA.items():
        nd = build()
        for lv in LEVELS:
            out[f"{name}_{lv[0]}"] = (oracle.validate([pol(*lv)], nd, nthreads=4), nd, lv)
    return out


@pytest.mark.parametrize("name", list(CORPORA))
def test_compact_against_oracle(compact, refs, oracle, name):
    for lv in LEVELS:
        key = f"{name}_{lv[0]}"
        ref, nd, _ = refs[key]
        for what in ("v", "cold", "m"):
            got = compact[f"{what}_{key}"]
            bad = np.argwhere(got != ref)
            assert bad.size == 0, (what, key, len(bad), bad[:5].tolist())
        assert np.array_equal(compact[f"cv_{key}"], want_masks(oracle, lv[0], lv[1], nd, ref)), key


@pytest.mark.parametrize("name", list(CORPORA))
def test_compact_equals_wide(compact, wide, name):
    """Bit for bit, and the two did read different columns: the wide launch's algorithmic bytes
    exceed the compact one's by 4 per pod and 4 per container."""
    for lv in LEVELS:
        key = f"{name}_{lv[0]}"
        for what in ("v", "cold", "m", "cv"):
            assert np.array_equal(compact[f"{what}_{key}"], wide[f"{what}_{key}"]), (what, key)
        n = compact[f"v_{key}"].shape[0]
        extra = float(wide[f"bytes_{key}"]) - float(compact[f"bytes_{key}"])
        assert extra >= 4.0 * n and extra % 4.0 == 0.0, (key, extra, n)
    if name == "capsets":
        assert float(wide["bytes_capsets_restricted"]) - float(compact["bytes_capsets_restricted"]) == 4.0 * 2100 + 4.0 * 2100


def test_batch_of_three_shards(compact, wide, refs):
    for name in BATCH:
        ref = refs[f"{name}_restricted"][0]
        assert np.array_equal(compact[f"b_{name}"], ref), (name, int((compact[f"b_{name}"] != ref).sum()))
        assert np.array_equal(wide[f"b_{name}"], ref), name


def test_corpora_hold_what_they_claim(refs):
    """The references themselves: the findings the corpora are built around are there."""
    rows = {o["metadata"]["name"]: i for i, o in enumerate(map(__import__("json").loads, clear_ndjson().splitlines()))}
    ref = refs["clear_restricted"][0]
    assert ref[rows["alone"], 0] == 2 and ref[rows["only0"], 0] == 1 and ref[rows["good0"], 0] == 1
    assert all(ref[rows[f"only{i}"], 0] == 2 for i in (1, 2, 3))
    base = refs["clear_baseline"][0]
    assert base[rows["only1"], 0] == 2 and base[rows["only3"], 0] == 1  # SYS_ADMIN added; a drop without ALL
    caps = refs["capsets_restricted"][0]
    assert caps[0, 0] == 1 and caps[1, 0] == 1 and caps[2047, 0] == 2 and caps[2048, 0] == 1
    assert refs["end_restricted"][0][:, 0].tolist() == [1, 1, 2]
    over = refs["overflow_restricted"][0]
    assert over[60, 0] == 2 and over[61, 0] == 1 and over[-1, 0] == 2 and over[-2, 0] == 1
    kinds = refs["kinds_restricted"][0]
    assert (kinds[-2] == 0).all() and (kinds[1] != 0).any() and kinds[1, 0] == 0  # ConfigMap: no rule; Deployment: autogen
