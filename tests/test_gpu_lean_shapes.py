"""The shapes kpe_lean6_kernel is compiled in, and what tells them apart.

The LEAN evaluation picks an instantiation from the program: whether it has the v1.0 seccomp check
(which reads the containers' seccomp annotations), and whether every versioned check has to be
decided (check masks per cell, or more than four version classes) or only the version classes
(one AND of the pod's evidence word with a mask per class). A staged container is one word: the
15 state bits the PSA checks read plus its capability-set code and seccomp-annotation bit. All of
it is held bit-exact to the oracle here: each instantiation on one corpus, the tile / wave / block
edges at 1, 2 and 4 tiles per wave, the verdict-only evaluation against the check-mask one, and
pods whose only finding is one container state bit."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import kyverno_amd as K
from tests.policies import pss_policy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAN6, BATCHED = 7, 9  # kpe_kernel_stats.scan_kernel: one-shard / multi-shard kpe_lean6_kernel launch
EDGE_SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1025)  # tile (64), wave (T x 64) and block (4 waves) edges


@pytest.fixture(scope="module")
def engine():
    return K.Engine(ordinal=0)


def pol(level, ver):
    return pss_policy(f"{level}-{ver.replace('.', '-')}", level, ver)


def stats_of(engine, run):
    engine.device.set_timing(True)
    engine.device.kernel_stats(reset=True)
    run()
    st = engine.device.kernel_stats(reset=True)
    engine.device.set_timing(False)
    return st


def want_masks(oracle, level, ver, nd, v):
    row = oracle.failing_cv_batch(level, ver, nd)
    return np.where(v == 2, np.maximum(row, 0)[:, None], 0).astype(np.int64)


def poison(engine, ps, c):
    hip = ctypes.CDLL("libamdhip64.so")
    ptr, nb = engine.device_verdicts(ps, c)
    assert hip.hipMemset(ctypes.c_void_p(ptr), 0xFF, ctypes.c_size_t(nb)) == 0
    assert hip.hipDeviceSynchronize() == 0


def test_instantiation_choice(engine, oracle):
    """One corpus with container seccomp annotations, evaluated alternately by a program that reads
    them (baseline v1.0) and one that does not (restricted latest), without and with check masks:
    four instantiations in turn on the same binding slots, then both programs through the
    multi-shard launch over poisoned verdicts."""
    from tests.golden.make_psum_digests import seccomp_ndjson
    nd = seccomp_ndjson(300)
    c = K.Corpus(nd, docs=False).upload(engine.device)
    c2 = K.Corpus(nd, docs=False).upload(engine.device)
    progs = [("baseline", "v1.0"), ("restricted", "latest")]
    sets = [K.PolicySet([pol(*lv)]) for lv in progs]
    refs = [oracle.validate([pol(*lv)], nd, nthreads=4) for lv in progs]
    assert (refs[0] == 2).any() and (refs[1] == 2).any()
    for _ in range(2):  # alternate: each program's launch follows the other's
        for (level, ver), ps, ref in zip(progs, sets, refs):
            for masks in (False, True):
                st = stats_of(engine, lambda: engine.evaluate_async(ps, c, masks=masks))
                assert st.launches == 1 and st.scan_kernel == LEAN6, (level, ver, masks, st.scan_kernel)
                v, _, _ = engine.fetch(ps, c, check_masks=masks)
                assert np.array_equal(v, ref), (level, ver, masks, int((v != ref).sum()))
                if masks:
                    got = engine.cv_masks(ps, c).astype(np.int64)
                    assert np.array_equal(got, want_masks(oracle, level, ver, nd, v)), (level, ver)
    for (level, ver), ps, ref in zip(progs, sets, refs):
        for masks in (False, True):
            for cc in (c, c2):
                engine.evaluate(ps, cc, check_masks=masks)
                poison(engine, ps, cc)
            st = stats_of(engine, lambda: engine.evaluate_batch_async(ps, [c, c2, c], masks=masks))
            assert st.launches == 1 and st.scan_kernel == BATCHED, (level, ver, masks, st.scan_kernel)
            engine.device.sync()
            for cc in (c, c2):
                v, _, _ = engine.fetch(ps, cc, check_masks=masks)
                assert np.array_equal(v, ref), (level, ver, masks)
                if masks:
                    got = engine.cv_masks(ps, cc).astype(np.int64)
                    assert np.array_equal(got, want_masks(oracle, level, ver, nd, v)), (level, ver)


# ---- tile, wave and block edges at every tiles-per-wave setting -------------------------------
def edge_ndjson(k):
    return K.synth_resources(0xED00 + k, EDGE_SIZES[k], mix=2)


def edge_child(tpw, out_path):
    """Runs in a process of its own (KPE_LEAN6_TPW is read when the device is opened): every edge
    size single-shard and all of them in one multi-shard launch, restricted latest, verdicts only
    and with check masks; writes what the device returned."""
    assert os.environ["KPE_LEAN6_TPW"] == str(tpw)
    eng = K.Engine(ordinal=0)
    ps = K.PolicySet([pol("restricted", "latest")])
    cs = [K.Corpus(edge_ndjson(k), docs=False).upload(eng.device) for k in range(len(EDGE_SIZES))]
    out = {}
    kinds, batch_kinds = [], []
    for masks in (False, True):
        for k, c in enumerate(cs):
            st = stats_of(eng, lambda: eng.evaluate_async(ps, c, masks=masks))
            kinds.append(st.scan_kernel)
            v, _, _ = eng.fetch(ps, c, check_masks=masks)
            out[f"one_{int(masks)}_{k}"] = v
            if masks:
                out[f"cv_{k}"] = eng.cv_masks(ps, c)
            poison(eng, ps, c)
        st = stats_of(eng, lambda: eng.evaluate_batch_async(ps, cs, masks=masks))
        batch_kinds.append((st.launches, st.scan_kernel))
        eng.device.sync()
        for k, c in enumerate(cs):
            out[f"batch_{int(masks)}_{k}"] = eng.fetch(ps, c, check_masks=masks)[0]
    out["kinds"], out["batch_kinds"] = np.asarray(kinds), np.asarray(batch_kinds)
    np.savez(out_path, **out)


@pytest.fixture(scope="module")
def edge_refs(oracle):
    p = [pol("restricted", "latest")]
    nds = [edge_ndjson(k) for k in range(len(EDGE_SIZES))]
    refs = [oracle.validate(p, nd, nthreads=4) for nd in nds]
    rows = [oracle.failing_cv_batch("restricted", "latest", nd) for nd in nds]
    return refs, rows


@pytest.mark.parametrize("tpw", [1, 2, 4])
def test_edges_tiles_per_wave(edge_refs, tmp_path, tpw):
    """n in {1, 63, 64, 65, 255, 256, 257, 1023, 1025} rows at 1, 2 and 4 tiles per wave (a fresh
    process and device per setting): a last tile, wave and block that are partial, full, or one row
    over; single-shard launches and all nine shards in one launch, whose blocks find their shard
    among nine."""
    refs, rows = edge_refs
    out = str(tmp_path / "edge.npz")
    env = dict(os.environ, KPE_LEAN6_TPW=str(tpw), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = f"from tests.test_gpu_lean_shapes import edge_child; edge_child({tpw}, {out!r})"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    assert (got["kinds"] == LEAN6).all(), got["kinds"].tolist()
    assert got["batch_kinds"].tolist() == [[1, BATCHED]] * 2, got["batch_kinds"].tolist()
    for k, n in enumerate(EDGE_SIZES):
        assert refs[k].shape == (n, 3)
        for name in (f"one_0_{k}", f"one_1_{k}", f"batch_0_{k}", f"batch_1_{k}"):
            assert np.array_equal(got[name], refs[k]), (tpw, n, name, int((got[name] != refs[k]).sum()))
        want = np.where(refs[k] == 2, np.maximum(rows[k], 0)[:, None], 0).astype(np.int64)
        assert np.array_equal(got[f"cv_{k}"].astype(np.int64), want), (tpw, n)


# ---- verdict-only evaluation against the check-mask evaluation -----------------------------------
MULTI = {
    # three version classes, R = 9: verdicts only decides classes by evidence masks
    "three-classes": [("restricted", "latest"), ("baseline", "v1.0"), ("restricted", "v1.22")],
    # five version classes, R = 15: more classes than evidence masks, every check decided
    "five-classes": [("restricted", "latest"), ("baseline", "v1.0"), ("restricted", "v1.22"), ("baseline", "latest"),
                     ("restricted", "v1.24")],
}


@pytest.fixture(scope="module")
def stress():
    from tests.test_gpu_lean import lean_stress_ndjson
    return lean_stress_ndjson(2000, 0x5A, unique_strings=False)


@pytest.mark.parametrize("name", list(MULTI))
def test_verdict_only_equals_masks(engine, oracle, stress, name):
    """Several podSecurity policies of different level / version in one set (ncls > 1, R > 4), on
    pods that take the kernel's slow paths: the verdict-only evaluation (classes by evidence masks,
    or by every check past four classes) and the check-mask evaluation (every check) give the same
    verdicts, the oracle's. Both sets take the LEAN path (asserted)."""
    pols = [pol(*lv) for lv in MULTI[name]]
    ps = K.PolicySet(pols)
    assert ps.num_rules == 3 * len(pols)
    c = K.Corpus(stress, docs=False).upload(engine.device)
    ref = oracle.validate(pols, stress, nthreads=4)
    st = stats_of(engine, lambda: engine.evaluate_async(ps, c))
    assert st.launches == 1 and st.scan_kernel == LEAN6, st.scan_kernel
    v, _, _ = engine.fetch(ps, c)
    poison(engine, ps, c)
    st = stats_of(engine, lambda: engine.evaluate_async(ps, c, masks=True))
    assert st.launches == 1 and st.scan_kernel == LEAN6, st.scan_kernel
    vm, _, _ = engine.fetch(ps, c, check_masks=True)
    assert np.array_equal(v, vm), int((v != vm).sum())
    bad = np.argwhere(v != ref)
    assert bad.size == 0, (len(bad), bad[:5].tolist())
    cv = engine.cv_masks(ps, c).astype(np.int64)
    for k, (level, ver) in enumerate(MULTI[name]):  # each policy's three columns hold its own checks
        cols = slice(3 * k, 3 * k + 3)
        assert np.array_equal(cv[:, cols], want_masks(oracle, level, ver, stress, vm[:, cols])), (level, ver)


# ---- the one-word container stage ------------------------------------------------------------------
GOOD_SC = {"allowPrivilegeEscalation": False, "capabilities": {"drop": ["ALL"]}, "runAsNonRoot": True,
           "seccompProfile": {"type": "RuntimeDefault"}}


def _sc(**kw):
    sc = json.loads(json.dumps(GOOD_SC))
    for k, val in kw.items():
        if val is None:
            sc.pop(k, None)
        else:
            sc[k] = val
    return sc


# one container finding per entry: the 15 container state bits the PSA checks read
BIT_CASES = {
    "priv_t": {"sc": _sc(privileged=True)},
    "ape_t": {"sc": _sc(allowPrivilegeEscalation=True)},
    "ape_u": {"sc": _sc(allowPrivilegeEscalation=None)},
    "rnr_f": {"sc": _sc(runAsNonRoot=False)},
    "rnr_u": {"sc": _sc(runAsNonRoot=None)},
    "rau_z": {"sc": _sc(runAsUser=0)},
    "sec_none": {"sc": _sc(seccompProfile=None)},
    "sec_unc": {"sc": _sc(seccompProfile={"type": "Unconfined"})},
    "sec_other": {"sc": _sc(seccompProfile={"type": "Bogus"})},
    "pm_other": {"sc": _sc(procMount="Unmasked")},
    "sel_other": {"sc": _sc(seLinuxOptions={"type": "spc_t"})},
    "sel_user": {"sc": _sc(seLinuxOptions={"type": "container_t", "user": "u"})},
    "sel_role": {"sc": _sc(seLinuxOptions={"type": "container_t", "role": "r"})},
    "whp_t": {"sc": _sc(windowsOptions={"hostProcess": True})},
    "hostport": {"sc": _sc(), "ports": [{"containerPort": 80, "hostPort": 8080}]},
}
CTR_COUNTS = (12, 5, 4, 1)  # the finding is on the last container: past the 4 clamped reads at 5 and 12


def stage_ndjson():
    """Pods whose only finding is one container state bit, on the last of 1, 4, 5 or 12 containers
    (the 12-container pods first: the first 64-pod tile holds 180 containers, past the 128 staged),
    the same pods without the finding, and pods with no containers at all."""
    out = []

    def pod(name, ctrs):
        out.append({"apiVersion": "v1", "kind": "Pod", "metadata": {"name": name, "namespace": "default"},
                    "spec": {"containers": ctrs}})

    for nc in CTR_COUNTS:
        for case, body in BIT_CASES.items():
            ctrs = [{"name": f"c{k}", "image": "nginx:1.0", "securityContext": _sc()} for k in range(nc - 1)]
            last = {"name": f"c{nc - 1}", "image": "nginx:1.0", "securityContext": body["sc"]}
            if "ports" in body:
                last["ports"] = body["ports"]
            pod(f"{case}-{nc}", ctrs + [last])
        pod(f"clean-{nc}", [{"name": f"c{k}", "image": "nginx:1.0", "securityContext": _sc()} for k in range(nc)])
        pod(f"empty-{nc}", [])
    return "\n".join(json.dumps(o, separators=(",", ":")) for o in out).encode()


@pytest.mark.parametrize("level,ver", [("restricted", "latest"), ("baseline", "v1.0")])
def test_one_word_container_stage(engine, oracle, level, ver):
    """Each of the 15 container state bits as a pod's only finding, with 0, 1, 4, 5 and 12
    containers and a tile of more than 128 containers: verdicts (verdict-only evaluation) and
    check masks equal the oracle's, and the finding decides the restricted verdict (the pods that
    differ only in it pass)."""
    nd = stage_ndjson()
    c = K.Corpus(nd, docs=False).upload(engine.device)
    assert c.n == len(CTR_COUNTS) * (len(BIT_CASES) + 2)
    ps = K.PolicySet([pol(level, ver)])
    ref = oracle.validate([pol(level, ver)], nd, nthreads=2)
    st = stats_of(engine, lambda: engine.evaluate_async(ps, c))
    assert st.launches == 1 and st.scan_kernel == LEAN6, st.scan_kernel
    v, _, _ = engine.fetch(ps, c)
    bad = np.argwhere(v != ref)
    assert bad.size == 0, (len(bad), bad[:5].tolist())
    vm, _, _ = engine.evaluate(ps, c, check_masks=True)
    assert np.array_equal(vm, ref)
    assert np.array_equal(engine.cv_masks(ps, c).astype(np.int64), want_masks(oracle, level, ver, nd, vm))
    if level == "restricted":  # every finding fails the Pod rule; the clean and the empty pods pass it
        per = len(BIT_CASES) + 2
        for g in range(len(CTR_COUNTS)):
            assert (ref[g * per:g * per + len(BIT_CASES), 0] == 2).all(), g
            assert (ref[g * per + len(BIT_CASES):(g + 1) * per, 0] == 1).all(), g
