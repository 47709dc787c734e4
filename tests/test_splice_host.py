"""Policy edits on a kept result, host half (no GPU): the column plan of kpe_results_splice
(kpe_splice_plan_names, the name-list form of kpe_splice_plan, which needs a kept result and so a
device) against the Python twin K.splice_plan and against plans written out by hand; the host
specification kpe_results_splice_host (K.splice_results) against the rule of include/kpe.h stated in
numpy and against the existing specification K.changed_rows over the full new matrix; and the pass
of the kernel (kyverno_amd/csrc/splice.inl) run lane by lane on the host under ASan / UBSan
(scripts/splice_check.cpp) over buffers of exactly N x Ro, N x Rs, N x rn and N bytes."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import kyverno_amd as K
from kyverno_amd._lib import load
from tests.conftest import build_host_tool

CODES = np.array([0, 1, 2, 3, 4, 5, 7], dtype=np.uint8)  # the kpe_verdict alphabet
KPE_E_INVALID, KPE_E_STATE = 1, 5


def c_plan(kept, sub, removed=()):
    """kpe_splice_plan_names: (plan, partner), or the negative status."""
    L = load()

    def arr(names):
        b = [n.encode() for n in names]
        return (ctypes.c_char_p * max(len(b), 1))(*b)

    ka, sa, ra = arr(kept), arr(sub), arr(removed)
    partner = np.zeros(max(len(sub), 1), dtype=np.int32)
    rn = L.kpe_splice_plan_names(ka, len(kept), sa, len(sub), ra, len(removed), None, partner.ctypes.data, 0)
    if rn < 0:
        return int(rn)
    plan = np.full(rn + 2, 77, dtype=np.int32)
    assert L.kpe_splice_plan_names(ka, len(kept), sa, len(sub), ra, len(removed), plan.ctypes.data, None, rn) == rn
    assert plan[rn:].tolist() == [77, 77]  # nothing past rn is written
    return plan[:rn], partner[:len(sub)]


def names(spec):
    """'a:3 b:1' -> ['a/r0', 'a/r1', 'a/r2', 'b/r0']"""
    return [f"{p}/r{i}" for p, k in (t.split(":") for t in spec.split()) for i in range(int(k))]


# (kept, sub, removed, the plan written out by hand)
PLAN_CASES = {
    "edited-first": ("a:2 b:1 c:1", "a:2", [], [-1, -2, 2, 3]),
    "edited-middle": ("a:2 b:1 c:1", "b:1", [], [0, 1, -1, 3]),
    "edited-last": ("a:2 b:1 c:1", "c:1", [], [0, 1, 2, -1]),
    "rules-3-to-1": ("a:1 b:3 c:1", "b:1", [], [0, -1, 4]),
    "rules-1-to-3": ("a:1 b:1 c:1", "b:3", [], [0, -1, -2, -3, 2]),
    "added": ("a:1 b:1", "n:2", [], [0, 1, -1, -2]),
    "removed": ("a:1 b:2 c:1", "", ["b"], [0, 3]),
    "two-edited": ("a:1 b:2 c:1 d:1", "d:2 b:1", [], [0, -3, 3, -1, -2]),
    "edited-added-removed": ("a:1 b:2 c:1", "n:1 c:2", ["a", "zz"], [1, 2, -2, -3, -1]),
    "whole-set": ("a:2 b:1", "a:2 b:1", [], [-1, -2, -3]),
    "nothing-kept": ("", "a:2", [], [-1, -2]),
}


@pytest.mark.parametrize("case", sorted(PLAN_CASES))
def test_plan_matches_the_twin_and_the_hand_written_plan(case):
    kept, sub, removed, want = PLAN_CASES[case]
    kept, sub = names(kept), names(sub)
    plan, partner = c_plan(kept, sub, removed)
    tplan, tpartner = K.splice_plan(kept, sub, removed)
    assert plan.tolist() == want and tplan.tolist() == want
    assert np.array_equal(partner, tpartner)
    assert partner.tolist() == [kept.index(n) if n in kept else -1 for n in sub]
    new_names = K.splice_names(kept, sub, plan)
    assert len(set(new_names)) == len(new_names)


def test_a_renamed_rule_of_an_edited_policy_has_no_partner():
    kept, sub = ["a/x", "b/old", "b/same"], ["b/same", "b/new"]
    plan, partner = c_plan(kept, sub)
    assert plan.tolist() == [0, -1, -2] and partner.tolist() == [2, -1]
    assert K.splice_names(kept, sub, plan) == ["a/x", "b/same", "b/new"]


@pytest.mark.parametrize("kept,sub,removed", [
    (["a/x", "b/y"], ["b/y"], ["b"]),  # removed and edited
    (["a/x", "a/x"], ["b/y"], []),  # a kept name twice
    (["a/x"], ["b/y", "b/y"], []),  # a sub name twice
], ids=["removed-and-edited", "kept-twice", "sub-twice"])
def test_plan_invalid(kept, sub, removed):
    assert c_plan(kept, sub, removed) == -KPE_E_INVALID
    with pytest.raises(K.KpeError) as e:
        K.splice_plan(kept, sub, removed)
    assert e.value.status == KPE_E_INVALID


def test_device_entry_points_check_arguments_and_state_first():
    L = load()
    assert L.kpe_results_splice(None, None, None, None, 0, None) == -KPE_E_INVALID
    assert L.kpe_spliced_rows(None, None, None, None, 0) == -KPE_E_INVALID
    assert L.kpe_splice_plan(None, None, None, 0, None, 0) == -KPE_E_INVALID
    corpus = K.Corpus([{"apiVersion": "v1", "kind": "Pod", "metadata": {"name": "a"}}])
    fake_dev = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    # not uploaded, nothing kept: no device call is reached
    assert L.kpe_spliced_rows(fake_dev, corpus.h, None, None, 0) == -KPE_E_STATE
    assert L.kpe_results_kept_fetch(fake_dev, corpus.h, 0, 1, None) == KPE_E_STATE
    assert K.splice_bytes(10, 3, 2, 4) == 100.0


# ---- the host specification ---------------------------------------------------------------------
def shape_plan(Ro, Rs, rn):
    """(plan, partner) of the named shape: the edits the GPU suite expresses."""
    if (Ro, Rs, rn) == (1, 1, 1):
        return [-1], [0]
    if (Ro, Rs, rn) == (3, 3, 3):  # the whole set edited
        return [-1, -2, -3], [0, 1, 2]
    if (Ro, Rs, rn) == (3, 3, 6):  # a policy of three rules added
        return [0, 1, 2, -1, -2, -3], [-1, -1, -1]
    if (Ro, Rs, rn) == (6, 3, 3):  # one policy removed, the other edited
        return [-1, -2, -3], [3, 4, 5]
    if (Ro, Rs, rn) == (18, 2, 15):  # a policy of two rules edited, one of three removed
        return list(range(5)) + [-1, -2] + list(range(10, 18)), [5, 6]
    if (Ro, Rs, rn) == (204, 1, 204):  # C3: one policy edited
        return list(range(90)) + [-1] + list(range(91, 204)), [90]
    if (Ro, Rs, rn) == (204, 3, 206):  # its rule replaced by three, one of them under the old name
        return list(range(90)) + [-1, -2, -3] + list(range(91, 204)), [-1, 90, -1]
    if (Ro, Rs, rn) == (4096, 1, 4096):
        return list(range(1000)) + [-1] + list(range(1001, 4096)), [1000]
    raise AssertionError((Ro, Rs, rn))


def matrices(seed, n, Ro, Rs, partner, p):
    """A seeded kept matrix over the alphabet, mostly NA like a real one, and an evaluation of sub
    that equals its partner columns (NA without one) but for a fraction p of redrawn cells."""
    rng = np.random.default_rng(seed)
    kept = rng.choice(CODES, size=(n, Ro), p=[0.7, 0.1, 0.1, 0.02, 0.03, 0.03, 0.02]).astype(np.uint8)
    if Ro > 100:  # a wide matrix: sparse, or every row has a response in a dropped column
        kept[rng.random((n, Ro)) < 0.9] = 0
    sub = np.zeros((n, Rs), dtype=np.uint8)
    for s in range(Rs):
        if partner[s] >= 0:
            sub[:, s] = kept[:, partner[s]]
    hit = rng.random((n, Rs)) < p
    sub[hit] = rng.choice(CODES, size=int(hit.sum()))
    return kept, sub


def spec_splice(kept, sub, plan, partner, always):
    n = kept.shape[0]
    out = np.zeros((n, len(plan)), dtype=np.uint8)
    for r, e in enumerate(plan):
        out[:, r] = kept[:, e] if e >= 0 else sub[:, -1 - e]
    pc = np.zeros_like(sub)
    for s, o in enumerate(partner):
        if o >= 0:
            pc[:, s] = kept[:, o]
    ch = (sub != pc).any(axis=1)
    ch |= (((always[None, :].astype(np.uint32) >> sub.astype(np.uint32)) & 1) != 0).any(axis=1)
    used = {int(e) for e in plan if e >= 0} | {int(o) for o in partner if o >= 0}
    gone = [o for o in range(kept.shape[1]) if o not in used]
    ch |= (kept[:, gone] != 0).any(axis=1)
    return out, ch.astype(np.uint8)


SHAPES = [(1, 1, 1), (3, 3, 3), (3, 3, 6), (6, 3, 3), (18, 2, 15), (204, 1, 204), (204, 3, 206), (4096, 1, 4096)]


def group_rows(Ro, Rs, rn):
    """The tiling of the pass (splice.inl splice_rows_per_group), restated: the library is not loaded
    while the tests are collected. test_tiling_constants holds it to kpe_splice_group_rows."""
    return max(1, min(1024, 4096 // max(Ro, Rs, rn, 1)))


def test_tiling_constants():
    L = load()
    for Ro, Rs, rn in SHAPES + [(0, 0, 0), (5000, 1, 1), (2, 7, 3)]:
        assert L.kpe_splice_group_rows(Ro, Rs, rn) == group_rows(Ro, Rs, rn)
    assert L.kpe_splice_max_groups() == 2048


def shape_rows(Ro, Rs, rn):
    """N = 1, 15, 16, 17, the group edge and its neighbours, and more groups than the blocks the
    harness runs (GRID), from the tiling constants of the pass."""
    rpg = group_rows(Ro, Rs, rn)
    return sorted({1, 15, 16, 17, rpg - 1, rpg, rpg + 1, (GRID + 1) * rpg + 2} - {0})


GRID = 2
CASES = [(s, n, a) for s in SHAPES for n in shape_rows(*s) for a in (0, 1)]


def case_inputs(shape, n, with_always):
    Ro, Rs, rn = shape
    plan, partner = (np.array(x, dtype=np.int32) for x in shape_plan(*shape))
    assert plan.shape == (rn,) and partner.shape == (Rs,)
    kept, sub = matrices(n * 31 + Ro, n, Ro, Rs, partner, p=0.05)
    always = np.full(Rs, K.MESSAGE_CODES if with_always else 0, dtype=np.uint8)
    return plan, partner, kept, sub, always


@pytest.fixture(scope="module")
def splice_check():
    return build_host_tool("splice_check")


@pytest.mark.parametrize("shape,n,with_always", CASES,
                         ids=[f"r{s[0]}-s{s[1]}-r{s[2]}-n{n}-{'always' if a else 'plain'}" for s, n, a in CASES])
def test_pass_under_asan_matches_the_twin(splice_check, tmp_path, shape, n, with_always):
    Ro, Rs, rn = shape
    plan, partner, kept, sub, always = case_inputs(shape, n, with_always)
    case, outp = tmp_path / "case.bin", tmp_path / "out.bin"
    with open(case, "wb") as f:
        f.write(struct.pack("<QIIII", n, Ro, Rs, rn, GRID))
        f.write(plan.tobytes() + partner.tobytes() + always.tobytes() + kept.tobytes() + sub.tobytes())
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([splice_check, str(case), str(outp)], env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    raw = np.fromfile(outp, dtype=np.uint8)
    got, gflags = raw[:n * rn].reshape(n, rn), raw[n * rn:]
    want, wflags, total = K.splice_results(kept, sub, plan, partner, always)
    assert np.array_equal(got, want), res.stdout
    assert np.array_equal(gflags, wflags), res.stdout
    assert total == int(wflags.sum())
    sout, sflags = spec_splice(kept, sub, plan, partner, always)
    assert np.array_equal(want, sout) and np.array_equal(wflags, sflags)
    if n * Rs >= 400 and not with_always:  # enough redrawn cells; neither no row nor every row
        assert 0 < total < n


@pytest.mark.parametrize("shape", SHAPES, ids=[f"r{a}-s{b}-r{c}" for a, b, c in SHAPES])
@pytest.mark.parametrize("with_always", [0, 1], ids=["plain", "always"])
def test_flags_are_changed_rows_of_the_full_matrix(shape, with_always):
    """The identity with the existing specification: the flags equal kpe_changed_rows' rule between
    K and the full new matrix K', mapped by name, `always` expanded to K''s columns."""
    n = 300
    plan, partner, kept, sub, always = case_inputs(shape, n, with_always)
    vb, flags, total = K.splice_results(kept, sub, plan, partner, always)
    cmap = np.array([e if e >= 0 else partner[-1 - e] for e in plan], dtype=np.int32)
    always_b = np.array([0 if e >= 0 else always[-1 - e] for e in plan], dtype=np.uint8)
    rows, vr, t = K.changed_rows(kept, vb, cmap, always_b)
    assert np.array_equal(rows, np.flatnonzero(flags).astype(np.uint64)) and t == total
    assert np.array_equal(vr, vb[rows.astype(np.int64)])


def test_host_twin_rejects_a_bad_plan():
    kept, sub = np.zeros((2, 3), np.uint8), np.zeros((2, 2), np.uint8)
    bad = [([0, 0, -1, -2], [-1, -1]),  # a kept column copied twice
           ([0, -1], [-1, -1]),  # a sub column left out
           ([0, -1, -1, -2], [-1, -1]),  # a sub column emitted twice
           ([0, -1, -2], [0, -1]),  # a copied column is also a partner
           ([3, -1, -2], [-1, -1]),  # past the kept rules
           ([-1, -2, -3], [-1, -1]),  # past the sub rules
           ([-1, -2], [1, 1])]  # a partner named twice
    for plan, partner in bad:
        with pytest.raises(K.KpeError) as e:
            K.splice_results(kept, sub, plan, partner)
        assert e.value.status == KPE_E_INVALID, (plan, partner)
    out, flags, total = K.splice_results(kept, sub, [2, -2, -1], [0, -1])
    assert out.shape == (2, 3) and total == 0 and not flags.any()
