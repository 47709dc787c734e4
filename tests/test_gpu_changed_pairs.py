"""The comparison across corpora on the device: kpe_changed_pairs and kpe_changed_pairs_fp against
the existing host twins over the gathered rows. Exact integer comparisons: the matrices themselves
are pinned to the oracle by the parity suites; these tests pin the pair comparison to the matrices.

Program A (12 rules) is evaluated and kept on an old corpus of 1,000 rows, program B (12 rules) is
evaluated on a new corpus of 300. B renames one policy of A (an explicit map pairs its rules), drops
one (its kept columns disappear) and adds one (no partner: -1). A wave of the kernels takes one pair
at a time and a block four; the pair lists are empty, one pair, 64 and 65 pairs (the wave / block and
tile-free edges of the compaction), a list that names one old row many times, and every new row
paired with a shuffled old row (75 blocks)."""
import copy
import ctypes
import functools

import numpy as np
import pytest

import kyverno_amd as K
from kyverno_amd._lib import load
from tests.policies import parity_policy_set, restricted_latest

pytestmark = pytest.mark.gpu

FAIL, ERROR, SKIP = 2, 4, 5
KPE_E_INVALID, KPE_E_STATE = 1, 5
N_OLD, N_NEW = 1000, 300


@pytest.fixture(scope="module")
def engine():
    return K.Engine(ordinal=0)


@functools.lru_cache(maxsize=None)
def programs():
    P = parity_policy_set()
    renamed = copy.deepcopy(P[1])
    renamed["metadata"]["name"] = P[1]["metadata"]["name"] + "-renamed"
    a = [restricted_latest(), P[1], P[2], P[3]]
    b = [P[3], renamed, P[5], restricted_latest()]  # P[2] dropped, P[5] added, the order changed
    return K.PolicySet(a), K.PolicySet(b), P[1]["metadata"]["name"]


@pytest.fixture(scope="module")
def state(engine):
    """A evaluated (with masks) and kept on the old corpus, both ways; B evaluated (with masks) on the
    new one. The matrices, mask words and kept fingerprints are fetched once and shared."""
    psa, psb, orig = programs()
    old = K.Corpus(K.synth_resources(21, N_OLD, mix=K.SYNTH_MIXED)).upload(engine.device)
    new = K.Corpus(K.synth_resources(22, N_NEW, mix=K.SYNTH_MIXED)).upload(engine.device)
    assert (old.n, new.n) == (N_OLD, N_NEW)
    engine.evaluate_async(psa, old, masks=True)
    va, _, _ = engine.fetch(psa, old)
    engine.keep_results(psa, old)
    st = {"psa": psa, "psb": psb, "old": old, "new": new, "va": va}
    # the map: by name, then the renamed policy's rules onto the original's
    cmap = K.column_map(psa.rule_names, psb.rule_names)
    for r, nm in enumerate(psb.rule_names):
        pol, rule = nm.split("/", 1)
        if pol == orig + "-renamed":
            cmap[r] = psa.rule_names.index(orig + "/" + rule)
    assert (cmap == -1).any() and len(set(range(psa.num_rules)) - set(cmap.tolist())) > 0
    st["cmap"] = cmap
    st["always"] = np.array([(K.SEL(FAIL) | K.SEL(ERROR) | K.SEL(SKIP))
                             if nm.split("/", 1)[0] == restricted_latest()["metadata"]["name"] else 0
                             for nm in psb.rule_names], dtype=np.uint8)
    assert st["always"].any() and not st["always"].all()
    engine.evaluate_async(psb, new, masks=True)
    st["vb"], _, _ = engine.fetch(psb, new)
    st["mb"] = engine.cv_masks(psb, new, raw=True)
    assert (st["vb"] == FAIL).any() and st["mb"].any()
    return st


def pair_lists():
    rng = np.random.default_rng(9)
    every = np.stack([np.arange(N_NEW), rng.permutation(N_OLD)[:N_NEW]], axis=1)
    rep = np.stack([rng.integers(0, N_NEW, 130), np.full(130, 417)], axis=1)
    rep[::3, 1] = 5  # two old rows, each named many times
    return {"empty": np.zeros((0, 2), dtype=np.uint64), "one": np.array([[N_NEW - 1, N_OLD - 1]]),
            "64": every[100:164], "65": every[37:102][::-1], "repeated-old": rep, "every-new-row": every}


LISTS = pair_lists()


def twin(st, pairs, cmap, always):
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    return K.changed_rows(st["va"][p[:, 1]], st["vb"][p[:, 0]], cmap, always)


@pytest.mark.parametrize("name", list(LISTS))
def test_changed_pairs_match_the_host_twin(engine, state, name):
    st, pairs = state, LISTS[name]
    for cmap, always in ((st["cmap"], st["always"]), (st["cmap"], 0),
                         (K.column_map(st["psa"].rule_names, st["psb"].rule_names), st["always"])):
        want_idx, want_vr, want_total = twin(st, pairs, cmap, always)
        for column_map in ((cmap,) if cmap is st["cmap"] else (None, cmap)):  # None: by name, built by the library
            idx, vr, total = engine.changed_pairs(st["psb"], st["new"], st["old"], pairs, column_map=column_map,
                                                  always=always)
            print(f"{name}: device {total}, twin {want_total} of {len(pairs)} pairs")
            assert total == want_total
            assert idx.dtype == np.uint64 and vr.shape == (want_total, st["psb"].num_rules)
            assert np.array_equal(idx, want_idx), np.setxor1d(idx, want_idx)[:8].tolist()
            assert np.array_equal(vr, want_vr)
    if name == "every-new-row":
        assert 0 < want_total <= N_NEW
        # without the verdict rows
        idx, vr, total = engine.changed_pairs(st["psb"], st["new"], st["old"], pairs, with_verdicts=False)
        assert total == idx.size and vr.shape == (0, st["psb"].num_rules)


def test_same_corpus_and_same_program_change_nothing(engine, state):
    """c_new == c_old: a corpus against its own kept result, row i with row i."""
    st = state
    engine.evaluate_async(st["psa"], st["old"], masks=True)
    ident = np.stack([np.arange(N_OLD), np.arange(N_OLD)], axis=1)
    idx, _, total = engine.changed_pairs(st["psa"], st["old"], st["old"], ident)
    assert total == 0 and idx.size == 0
    # row i with row j: the twin's answer
    rng = np.random.default_rng(3)
    pairs = np.stack([rng.integers(0, N_OLD, 500), rng.integers(0, N_OLD, 500)], axis=1)
    ident_map = np.arange(st["psa"].num_rules, dtype=np.int32)
    want_idx, want_vr, want_total = K.changed_rows(st["va"][pairs[:, 1]], st["va"][pairs[:, 0]], ident_map)
    idx, vr, total = engine.changed_pairs(st["psa"], st["old"], st["old"], pairs)
    assert total == want_total > 0 and np.array_equal(idx, want_idx) and np.array_equal(vr, want_vr)


@pytest.mark.parametrize("masks", [False, True], ids=["verdicts", "fp-masks"])
@pytest.mark.parametrize("name", list(LISTS))
def test_changed_pairs_fp_match_the_host_twin(engine, state, name, masks):
    st, pairs = state, LISTS[name]
    psa, psb = st["psa"], st["psb"]
    engine.evaluate_async(psa, st["old"], masks=True)  # the old corpus may hold another evaluation by now
    engine.keep_fingerprints(psa, st["old"], masks=masks)
    kept = engine.kept_fingerprints(st["old"])
    salts = K.rule_salts(psb)
    msg = salts ^ np.where(st["always"] != 0, np.uint64(3), np.uint64(0))  # an edit counter on one policy
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    fp_new = K.row_fingerprints(st["vb"][p[:, 0]], salts, msg_salts=msg, cv_masks=st["mb"][p[:, 0]] if masks else None)
    want_idx = np.flatnonzero(fp_new != kept[p[:, 1]]).astype(np.uint64)
    idx, vr, fps, total = engine.changed_pairs_fp(psb, st["new"], st["old"], pairs, msg_salts=msg, masks=masks)
    print(f"{name}: device {total}, twin {want_idx.size} of {len(pairs)} pairs")
    assert total == want_idx.size and np.array_equal(idx, want_idx)
    assert np.array_equal(vr, st["vb"][p[want_idx.astype(np.int64), 0]])
    assert np.array_equal(fps, fp_new[want_idx.astype(np.int64)])
    # explicit default salts are the default
    idx2, _, _, t2 = engine.changed_pairs_fp(psb, st["new"], st["old"], pairs, salts=salts, msg_salts=msg, masks=masks)
    assert t2 == total and np.array_equal(idx2, idx)
    if name == "every-new-row":
        assert 0 < total <= N_NEW
        # the fingerprints equal: the same program on the same rows
        engine.keep_fingerprints(psb, st["new"], msg_salts=msg, masks=masks)
        ident = np.stack([np.arange(N_NEW), np.arange(N_NEW)], axis=1)
        assert engine.changed_pairs_fp(psb, st["new"], st["new"], ident, msg_salts=msg, masks=masks)[3] == 0
        engine.drop_fingerprints(st["new"])


def test_cap_writes_exactly_cap_entries(engine, state):
    st, pairs = state, np.ascontiguousarray(LISTS["every-new-row"], dtype=np.uint64)
    L = load()
    Rn = st["psb"].num_rules
    want_idx, want_vr, total = twin(st, pairs, st["cmap"], st["always"])
    assert total > 20
    h = (engine.device.h, st["psb"].h, st["new"].h, st["old"].h, pairs.ctypes.data, len(pairs))
    cm, al = st["cmap"].ctypes.data, st["always"].ctypes.data
    assert L.kpe_changed_pairs(*h, cm, al, None, None, 0) == total  # count only
    cap = total // 2
    idx = np.full(total + 8, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    vr = np.full((total + 8, Rn), 0xA5, dtype=np.uint8)
    assert L.kpe_changed_pairs(*h, cm, al, idx.ctypes.data, vr.ctypes.data, cap) == total
    assert np.array_equal(idx[:cap], want_idx[:cap]) and np.array_equal(vr[:cap], want_vr[:cap])
    assert (idx[cap:] == np.uint64(0xDEADBEEFDEADBEEF)).all() and (vr[cap:] == 0xA5).all()
    i2, v2, t2 = engine.changed_pairs(st["psb"], st["new"], st["old"], pairs, column_map=st["cmap"], always=st["always"],
                                      cap=cap)
    assert t2 == total and np.array_equal(i2, want_idx[:cap]) and np.array_equal(v2, want_vr[:cap])
    # the fingerprint form
    engine.evaluate_async(st["psa"], st["old"], masks=True)
    engine.keep_fingerprints(st["psa"], st["old"])
    _, _, _, tfp = engine.changed_pairs_fp(st["psb"], st["new"], st["old"], pairs)
    assert tfp > 4
    fps = np.full(tfp + 4, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    idx[:] = np.uint64(0xDEADBEEFDEADBEEF)
    assert L.kpe_changed_pairs_fp(*h, None, None, K.MESSAGE_CODES, 0, idx.ctypes.data, None, fps.ctypes.data, 3) == tfp
    assert (idx[:3] != np.uint64(0xDEADBEEFDEADBEEF)).all() and (idx[3:] == np.uint64(0xDEADBEEFDEADBEEF)).all()
    assert (fps[:3] != np.uint64(0xDEADBEEFDEADBEEF)).all() and (fps[3:] == np.uint64(0xDEADBEEFDEADBEEF)).all()
    # a row past its corpus, a map the kept result does not have
    bad = pairs.copy()
    bad[7, 0] = N_NEW
    assert L.kpe_changed_pairs(engine.device.h, st["psb"].h, st["new"].h, st["old"].h, bad.ctypes.data, len(bad), cm, al,
                               None, None, 0) == -KPE_E_INVALID
    badmap = st["cmap"].copy()
    badmap[0] = st["psa"].num_rules
    assert L.kpe_changed_pairs(*h, badmap.ctypes.data, al, None, None, 0) == -KPE_E_INVALID


def test_state_errors(engine):
    psa, psb, _ = programs()
    old = K.Corpus(K.synth_resources(21, 64, mix=K.SYNTH_MIXED)).upload(engine.device)
    new = K.Corpus(K.synth_resources(22, 32, mix=K.SYNTH_MIXED)).upload(engine.device)
    pairs = np.array([[0, 0], [31, 63]])

    def refused(f):
        with pytest.raises(K.KpeError) as e:
            f()
        assert e.value.status == KPE_E_STATE

    both = (lambda: engine.changed_pairs(psb, new, old, pairs), lambda: engine.changed_pairs_fp(psb, new, old, pairs))
    engine.evaluate_async(psb, new)
    for f in both:
        refused(f)  # the old corpus keeps nothing
    engine.evaluate_async(psa, old)
    engine.keep_results(psa, old)
    engine.keep_fingerprints(psa, old)
    for f in both:
        f()
    engine.evaluate_async(psa, new)
    for f in both:
        refused(f)  # the new corpus holds another program's evaluation
    refused(lambda: engine.changed_pairs_fp(psa, new, old, pairs, masks=True))  # masks were not written
    not_up = K.Corpus(K.synth_resources(22, 32, mix=K.SYNTH_MIXED))
    refused(lambda: engine.changed_pairs(psa, not_up, old, pairs))


def test_a_corpus_of_another_device_is_refused(engine):
    ndev = ctypes.c_int(0)
    assert ctypes.CDLL("libamdhip64.so").hipGetDeviceCount(ctypes.byref(ndev)) == 0
    if ndev.value < 2:
        pytest.skip("one device: no corpus of another device to refuse")
    psa, psb, _ = programs()
    new = K.Corpus(K.synth_resources(22, 32, mix=K.SYNTH_MIXED)).upload(engine.device)
    pairs = np.array([[0, 0], [31, 63]])

    def refused(f):
        with pytest.raises(K.KpeError) as e:
            f()
        assert e.value.status == KPE_E_STATE

    other = K.Engine(ordinal=1)
    far = K.Corpus(K.synth_resources(21, 64, mix=K.SYNTH_MIXED)).upload(other.device)
    other.evaluate_async(psa, far)
    other.keep_results(psa, far)
    other.keep_fingerprints(psa, far)
    engine.evaluate_async(psb, new)
    for f in (lambda: engine.changed_pairs(psb, new, far, pairs), lambda: engine.changed_pairs_fp(psb, new, far, pairs)):
        refused(f)
