"""kpe_lean6_kernel's tile body on hand-built corpora: what a shorter instruction stream can break.

Every case compares the full verdict matrix with the oracle, and the check-mask evaluation (every
versioned check) with the verdict-only one (evidence word, pod-evidence table). The corpora are
built pod by pod so that an item's place in its tile's stage is known: partial last tiles and
waves whose later tiles do not exist, list items at every byte alignment between offending
neighbours, containers at every one of the four word reads and at the stage's edge (128 containers
in a tile, and 129), one pod per value of each pod-level field, and one launch over three shards."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import kyverno_amd as K
from tests.test_gpu_lean_shapes import BATCHED, LEAN6, _sc, poison, pol, stats_of, want_masks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_COUNTS = (1, 63, 64, 65, 255, 257)
# container bodies without the fields a pod-level securityContext can supply
NEUTRAL_SC = {"allowPrivilegeEscalation": False, "capabilities": {"drop": ["ALL"]}}
GOOD_POD_SC = {"runAsNonRoot": True, "seccompProfile": {"type": "RuntimeDefault"}}


@pytest.fixture(scope="module")
def engine():
    return K.Engine(ordinal=0)


def ctr(k, sc=None):
    return {"name": f"c{k}", "image": "nginx:1.0", "securityContext": _sc() if sc is None else sc}


def pod(name, ctrs=None, vols=(), sysctls=(), ann=None, psc=None, **spec):
    s = {"containers": [ctr(0)] if ctrs is None else ctrs}
    if vols:
        s["volumes"] = [{"name": f"v{k}", **v} for k, v in enumerate(vols)]
    sc = dict(psc or {})
    if sysctls:
        sc["sysctls"] = [{"name": nm, "value": "1"} for nm in sysctls]
    if sc:
        s["securityContext"] = sc
    s.update(spec)
    meta = {"name": name, "namespace": "default"}
    if ann:
        meta["annotations"] = ann
    return {"apiVersion": "v1", "kind": "Pod", "metadata": meta, "spec": s}


def controller(kind, name, ctrs):
    """A workload of a controller kind whose pod template holds the containers `ctrs`."""
    tmpl = {"metadata": {"labels": {"app": "w"}}, "spec": {"containers": ctrs}}
    if kind == "CronJob":
        spec = {"schedule": "* * * * *", "jobTemplate": {"spec": {"template": tmpl}}}
        api = "batch/v1"
    else:
        spec = {"selector": {"matchLabels": {"app": "w"}}, "template": tmpl}
        api = "apps/v1"
    return {"apiVersion": api, "kind": kind, "metadata": {"name": name, "namespace": "default"}, "spec": spec}


def ndjson(pods):
    return "\n".join(json.dumps(o, separators=(",", ":")) for o in pods).encode()


def check(engine, oracle, nd, levels=(("restricted", "latest"),)):
    """Verdicts (verdict-only launch) and check masks against the oracle; returns the references."""
    c = K.Corpus(nd, docs=False).upload(engine.device)
    refs = []
    for level, ver in levels:
        p = pol(level, ver)
        ps = K.PolicySet([p])
        ref = oracle.validate([p], nd, nthreads=4)
        st = stats_of(engine, lambda: engine.evaluate_async(ps, c))
        assert st.launches == 1 and st.scan_kernel == LEAN6, st.scan_kernel
        v, _, _ = engine.fetch(ps, c)
        bad = np.argwhere(v != ref)
        assert bad.size == 0, (level, ver, len(bad), bad[:5].tolist())
        poison(engine, ps, c)
        vm, _, _ = engine.evaluate(ps, c, check_masks=True)
        assert np.array_equal(vm, v), (level, ver, int((vm != v).sum()))
        assert np.array_equal(engine.cv_masks(ps, c).astype(np.int64), want_masks(oracle, level, ver, nd, vm)), (level, ver)
        refs.append(ref)
    return refs


# ---- row counts ---------------------------------------------------------------------------------
def rows_ndjson(n):
    """n pods, each seventh with a finding of another kind, the last one always offending."""
    out = []
    for i in range(n):
        k = i % 7 if i < n - 1 else 1
        if k == 1:
            out.append(pod(f"p{i}", [ctr(0, _sc(privileged=True))]))
        elif k == 3:
            out.append(pod(f"p{i}", vols=[{"hostPath": {"path": "/x"}}]))
        elif k == 5:
            out.append(pod(f"p{i}", psc={"runAsUser": 0}))
        else:
            out.append(pod(f"p{i}", vols=[{"emptyDir": {}}] * (i % 3)))
    return ndjson(out)


@pytest.fixture(scope="module")
def row_refs(oracle):
    p = [pol("restricted", "latest")]
    return [oracle.validate(p, rows_ndjson(n), nthreads=4) for n in ROW_COUNTS]


@pytest.mark.parametrize("k", range(len(ROW_COUNTS)))
def test_row_counts(engine, oracle, k):
    """n = 1, 63, 64, 65, 255, 257: a partial last tile, a full one, one row over."""
    ref, = check(engine, oracle, rows_ndjson(ROW_COUNTS[k]))
    assert ref.shape == (ROW_COUNTS[k], 3) and ref[-1, 0] == 2


def rows_child(tpw, out_path):
    """In a process of its own (KPE_LEAN6_TPW is read when the device is opened): every row count,
    verdicts only and with check masks."""
    assert os.environ["KPE_LEAN6_TPW"] == str(tpw)
    eng = K.Engine(ordinal=0)
    ps = K.PolicySet([pol("restricted", "latest")])
    out = {}
    for k, n in enumerate(ROW_COUNTS):
        c = K.Corpus(rows_ndjson(n), docs=False).upload(eng.device)
        eng.evaluate_async(ps, c)
        out[f"v_{k}"] = eng.fetch(ps, c)[0]
        poison(eng, ps, c)
        out[f"m_{k}"] = eng.evaluate(ps, c, check_masks=True)[0]
    np.savez(out_path, **out)


@pytest.mark.parametrize("tpw", [1, 2, 4])
def test_row_counts_tiles_per_wave(row_refs, tmp_path, tpw):
    """The same corpora at 1, 2 and 4 tiles per wave: at 4, the wave of the 65-row corpus has two
    tiles that exist and two that do not, the 1-row corpus one and three."""
    out = str(tmp_path / "rows.npz")
    env = dict(os.environ, KPE_LEAN6_TPW=str(tpw), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = f"from tests.test_gpu_lean_stream import rows_child; rows_child({tpw}, {out!r})"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    for k, n in enumerate(ROW_COUNTS):
        for name in (f"v_{k}", f"m_{k}"):
            assert np.array_equal(got[name], row_refs[k]), (tpw, n, name, int((got[name] != row_refs[k]).sum()))


# ---- list items at every byte alignment ------------------------------------------------------------
LISTS = {
    # list: (clean item, offending items, most items of a target pod)
    "vol": ({"emptyDir": {}}, [{"hostPath": {"path": "/x"}}, {"nfs": {"server": "s", "path": "/"}}], 5),
    "sys": ("kernel.shm_rmid_forced", ["kernel.msgmax"], 3),
    "ann": (("note{}", "v"), [("container.apparmor.security.beta.kubernetes.io/c0", "unconfined")], 3),
}


def list_pod(kind, name, items):
    if kind == "vol":
        return pod(name, vols=items)
    if kind == "sys":
        return pod(name, sysctls=items)
    # every annotation of the pod is a list item, in document order (flatten.cpp keeps pod.ann as
    # read; json.dumps keeps the dict's order), so distinct keys give len(items) items in this order
    ann = {k.format(i): v for i, (k, v) in enumerate(items)}
    assert len(ann) == len(items) and list(ann.values()) == [v for _, v in items]
    return pod(name, ann=ann)


def align_ndjson(kind):
    """Groups of four pods (a filler that sets the alignment, an offending neighbour, the target,
    an offending neighbour) for every alignment 0-3 of the target's first item in its tile's
    stage, every item count of the target and its offending item first, last or absent. A tile
    holds whole groups."""
    good, bads, most = LISTS[kind]
    pods, targets, off = [], [], 0  # off: items of this tile so far

    def add(p, n_items):
        nonlocal off
        if len(pods) % 64 == 0:
            off = 0
        pods.append(p)
        off += n_items

    for bad in bads:
        for a in range(4):
            for cnt in range(most + 1):
                for where in ("none", "first", "last"):
                    if where != "none" and cnt == 0:
                        continue
                    i = len(pods)  # a multiple of 4: a group never straddles two tiles
                    if i % 64 == 0:
                        off = 0
                    fill = (a - (off + 1)) % 4
                    add(list_pod(kind, f"f{i}", [good] * fill), fill)
                    add(list_pod(kind, f"l{i}", [bad]), 1)
                    assert off % 4 == a
                    items = [good] * cnt
                    if where == "first":
                        items[0] = bad
                    elif where == "last":
                        items[-1] = bad
                    targets.append((len(pods), where != "none"))
                    add(list_pod(kind, f"t{i}", items), cnt)
                    add(list_pod(kind, f"r{i}", [bad]), 1)
    return ndjson(pods), targets


@pytest.mark.parametrize("kind", list(LISTS))
def test_list_alignment(engine, oracle, kind):
    """Volumes (0-5 per pod), sysctls and annotations (0-3) at stage offsets = 0, 1, 2, 3 (mod 4),
    the pod's offending item first, last or absent, both neighbours offending: a neighbour's byte
    read as the pod's own flips a verdict. restricted latest and baseline latest (hostPath fails
    both, nfs the restricted volume types only)."""
    nd, targets = align_ndjson(kind)
    refs = check(engine, oracle, nd, (("restricted", "latest"), ("baseline", "latest")))
    ref = refs[0]
    for row, offending in targets:
        assert (ref[row, 0] == 2) == offending, (kind, row, offending)
        assert ref[row - 1, 0] == 2 and ref[row + 1, 0] == 2, (kind, row)


# ---- containers at each of the four reads, and the stage's edge ------------------------------------
def ctr_ndjson():
    """Pods of 0, 1, 4 and 5 containers with the offending one at each position or absent, between
    offending neighbours; then a tile of exactly 128 containers and one of 129, each with its
    last pod's last container offending."""
    pods, targets = [], []
    bad_sc = _sc(privileged=True)
    for nc in (0, 1, 4, 5):
        for at in [None] + list(range(nc)):
            pods.append(pod(f"l{len(pods)}", [ctr(0, bad_sc)]))
            targets.append((len(pods), at is not None))
            pods.append(pod(f"t{len(pods)}", [ctr(k, bad_sc if k == at else None) for k in range(nc)]))
            pods.append(pod(f"r{len(pods)}", [ctr(0, bad_sc)]))
    # controller kinds: rows whose kind the Pod rule does not match and whose template has no
    # container (0 containers through the kind table), and the same kinds with an offending one,
    # between offending pods
    for kind in ("Deployment", "DaemonSet", "CronJob"):
        for bad in (False, True):
            pods.append(pod(f"l{len(pods)}", [ctr(0, bad_sc)]))
            targets.append((len(pods), None))
            pods.append(controller(kind, f"w{len(pods)}", [ctr(0, bad_sc)] if bad else []))
            pods.append(pod(f"r{len(pods)}", [ctr(0, bad_sc)]))
    while len(pods) % 64:
        pods.append(pod(f"fill{len(pods)}", []))
    for extra in (0, 1):  # 64 x 2 containers, then 63 x 2 + 3
        for i in range(64):
            nc = 2 + (extra if i == 63 else 0)
            last = i == 63
            targets.append((len(pods), last))
            pods.append(pod(f"e{extra}-{i}", [ctr(k, bad_sc if last and k == nc - 1 else None) for k in range(nc)]))
    return ndjson(pods), targets


def test_container_reads(engine, oracle):
    nd, targets = ctr_ndjson()
    ref, _ = check(engine, oracle, nd, (("restricted", "latest"), ("baseline", "v1.0")))
    for row, offending in targets:
        if offending is None:  # a controller row: the Pod rule does not apply, an autogen rule does
            assert ref[row, 0] == 0 and (ref[row] != 0).any(), (row, ref[row].tolist())
        else:
            assert (ref[row, 0] == 2) == offending, (row, offending)


# ---- one pod per value of each pod-level field ---------------------------------------------------
def podword_ndjson():
    pods = []

    def add(name, psc=None, **spec):
        pods.append(pod(f"{name}-{len(pods)}", [ctr(0, dict(NEUTRAL_SC))], psc={**GOOD_POD_SC, **(psc or {})}, **spec))

    add("neutral")
    for key in ("hostNetwork", "hostPID", "hostIPC"):
        for val in (True, False):
            add(key, **{key: val})
    for val in (True, False):
        add("rnr", {"runAsNonRoot": val})
    add("rnr-unset")
    pods[-1]["spec"]["securityContext"].pop("runAsNonRoot")
    for val in (0, 1000):
        add("rau", {"runAsUser": val})
    for typ in ("RuntimeDefault", "Localhost", "Unconfined", "Bogus", ""):
        prof = {"type": typ}
        if typ == "Localhost":
            prof["localhostProfile"] = "p.json"
        add("seccomp", {"seccompProfile": prof})
    add("seccomp-unset")
    pods[-1]["spec"]["securityContext"].pop("seccompProfile")
    for typ in ("", "container_t", "container_init_t", "container_kvm_t", "spc_t"):
        for extra in ({}, {"user": "u"}, {"role": "r"}, {"user": "u", "role": "r"}):
            add("sel", {"seLinuxOptions": {"type": typ, **extra}})
    add("sel-user-only", {"seLinuxOptions": {"user": "u"}})
    for val in (True, False):
        add("whp", {"windowsOptions": {"hostProcess": val}}, hostNetwork=val)
    for os_name in ("windows", "linux"):
        add("os", os={"name": os_name})
        # a Windows pod is spared the checks that do not apply to it: leave their fields unset
        pods.append(pod(f"os-bare-{len(pods)}", [ctr(0, {})], os={"name": os_name}))
    return ndjson(pods)


@pytest.mark.parametrize("level,ver", [("restricted", "v1.0"), ("restricted", "v1.25"), ("restricted", "latest"),
                                       ("baseline", "v1.0"), ("baseline", "v1.25"), ("baseline", "latest")])
def test_pod_word_fields(engine, oracle, level, ver):
    """Host namespaces, runAsNonRoot, runAsUser, the seccomp types, the SELinux types with and
    without user / role, hostProcess and the OS name, one pod per value with the other fields
    neutral, under the restricted and baseline versions that differ."""
    ref, = check(engine, oracle, podword_ndjson(), ((level, ver),))
    assert (ref[:, 0] == 1).any() and (ref[:, 0] == 2).any()


# ---- one launch over three shards -----------------------------------------------------------------
def test_batch_of_three_shards(engine, oracle):
    """65, 4096 and 257 rows in one launch (blocks find their shard; the last tiles are partial)."""
    p = pol("restricted", "latest")
    ps = K.PolicySet([p])
    nds = [rows_ndjson(n) for n in (65, 4096, 257)]
    cs = [K.Corpus(nd, docs=False).upload(engine.device) for nd in nds]
    refs = [oracle.validate([p], nd, nthreads=4) for nd in nds]
    for masks in (False, True):
        for c in cs:
            engine.evaluate(ps, c, check_masks=masks)
            poison(engine, ps, c)
        st = stats_of(engine, lambda: engine.evaluate_batch_async(ps, cs, masks=masks))
        assert st.launches == 1 and st.scan_kernel == BATCHED, st.scan_kernel
        engine.device.sync()
        for c, nd, ref in zip(cs, nds, refs):
            v, _, _ = engine.fetch(ps, c, check_masks=masks)
            assert np.array_equal(v, ref), (masks, ref.shape, int((v != ref).sum()))
            if masks:
                assert np.array_equal(engine.cv_masks(ps, c).astype(np.int64),
                                      want_masks(oracle, "restricted", "latest", nd, v))
