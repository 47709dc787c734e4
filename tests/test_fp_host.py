"""Row fingerprints, host half (no GPU): the entry points are exported, the host twin
(kpe_row_fingerprints_host) equals the specification of include/kpe.h restated in numpy on uint64
arrays, the properties the header states hold (column order, NA columns, the empty row, one cell, the
mask word, the message salts), kpe_fp_rule_salts is FNV-1a-64 + mix64 of the rule names, the rows whose
fingerprints differ are exactly the rows the exact form (kpe_changed_rows_host) reports, the argument
checks of the device entry points come before any device call, and the kernel's body
(kyverno_amd/csrc/fp.inl) run lane by lane on the host under ASan / UBSan (scripts/fp_check.cpp) gives
the twin's fingerprints at every shape the GPU suite uses."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import kyverno_amd as K
from kyverno_amd._lib import load
from tests.conftest import build_host_tool
from tests.policies import pss_policy, restricted_latest
from tests.test_delta_host import CODES, SHAPES as DELTA_SHAPES, maps, matrices

KPE_E_INVALID, KPE_E_LIMIT, KPE_E_STATE = 1, 4, 5
FAIL = 2
U = np.uint64
GOLD, M1, M2 = U(0x9E3779B97F4A7C15), U(0xBF58476D1CE4E5B9), U(0x94D049BB133111EB)


def mix64(z):
    """The splitmix64 finaliser on a uint64 array (wrapping)."""
    z = np.array(z, dtype=U)
    z ^= z >> U(30)
    z *= M1
    z ^= z >> U(27)
    z *= M2
    z ^= z >> U(31)
    return z


def spec_fp(v, salts, msg_salts=None, msg_codes=0, masks=None):
    """fp(i) = sum over the cells v != NA of mix64(S(r, v) + GOLD * (v | m << 8)), on uint64."""
    v = np.asarray(v, dtype=np.uint8)
    salts = np.asarray(salts, dtype=U)
    msg_salts = salts if msg_salts is None else np.asarray(msg_salts, dtype=U)
    v64 = v.astype(U)
    is_msg = ((U(msg_codes) >> np.minimum(v64, U(63))) & U(1)) != 0
    S = np.where(is_msg, msg_salts[None, :], salts[None, :])
    m = np.zeros(v.shape, dtype=U) if masks is None else np.where(v == FAIL, masks, 0).astype(U)
    h = mix64(S + GOLD * (v64 | (m << U(8))))
    h[v == 0] = 0
    return h.sum(axis=1, dtype=U)


def fnv1a64(name):
    h = 0xCBF29CE484222325
    for b in name.encode():
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def name_salts(names):
    s = mix64(np.array([fnv1a64(n) for n in names], dtype=U))
    s[s == 0] = 1
    return s


def matrix(seed, n, R):
    """A seeded matrix over the alphabet, mostly NA: the kept side of test_delta_host.matrices."""
    return matrices(seed, n, R, R, np.arange(R, dtype=np.int32))[0]


def rand_salts(seed, R):
    return np.random.default_rng(seed).integers(1, 1 << 63, size=R, dtype=np.uint64) * U(2) + U(1)


def rand_masks(seed, shape):
    """Mask words on every cell, bit 31 included: the words of non-FAIL cells must be ignored."""
    return np.random.default_rng(seed).integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)


def test_symbols_exported():
    L = load()
    for name in ("kpe_fp_rule_salts", "kpe_fetch_row_fingerprints", "kpe_row_fingerprints_host",
                 "kpe_fingerprints_keep", "kpe_fingerprints_load", "kpe_fingerprints_fetch", "kpe_fingerprints_drop",
                 "kpe_fingerprints_kept", "kpe_changed_rows_fp", "kpe_changed_fingerprints_host"):
        assert hasattr(L, name), name
    for name in ("rule_salts", "row_fingerprints", "changed_fingerprints"):
        assert callable(getattr(K, name)), name
    for name in ("row_fingerprints", "keep_fingerprints", "load_fingerprints", "kept_fingerprints", "changed_rows_fp"):
        assert callable(getattr(K.Engine, name)), name
    assert K.MESSAGE_CODES == K.ResidentScanner.MESSAGE_CODES == K.SEL(2) | K.SEL(4) | K.SEL(5)
    assert int(mix64([0])[0]) == 0


TWIN_SHAPES = [(0, 3), (1, 1), (17, 1), (300, 3), (257, 18), (64, 204), (5, 4096)]


@pytest.mark.parametrize("n,R", TWIN_SHAPES, ids=[f"n{n}-r{r}" for n, r in TWIN_SHAPES])
def test_host_twin_matches_the_specification(n, R):
    v = matrix(n * 31 + R, n, R)
    salts, msg_salts = rand_salts(R, R), rand_salts(R + 1000, R)
    masks = rand_masks(n + R, (n, R))
    for msg_codes in [0, K.MESSAGE_CODES] + [1 << b for b in range(8)]:
        for mk in (None, masks):
            want = spec_fp(v, salts, msg_salts, msg_codes, mk)
            got = K.row_fingerprints(v, salts, msg_salts=msg_salts, msg_codes=msg_codes, cv_masks=mk)
            assert got.dtype == np.uint64 and got.shape == (n,)
            assert np.array_equal(got, want), (msg_codes, mk is not None)
    # msg_salts == NULL means salts, whatever msg_codes says
    assert np.array_equal(K.row_fingerprints(v, salts, msg_codes=0xFF), spec_fp(v, salts))
    if n:  # as many fingerprints as distinct rows: seeded, so a collision would show here
        assert np.unique(K.row_fingerprints(v, salts)).size == np.unique(v, axis=0).shape[0]


def test_column_order_and_na_columns_do_not_matter():
    n, R = 300, 18
    v = matrix(3, n, R)
    salts, msg_salts, masks = rand_salts(1, R), rand_salts(2, R), rand_masks(4, (n, R))
    base = K.row_fingerprints(v, salts, msg_salts=msg_salts, cv_masks=masks)
    perm = np.random.default_rng(5).permutation(R)
    assert np.array_equal(K.row_fingerprints(v[:, perm], salts[perm], msg_salts=msg_salts[perm], cv_masks=masks[:, perm]),
                          base)
    # all-NA columns inserted (a policy that matches nothing), with any salts and any mask words
    at = [0, 0, 7, R]
    v2 = np.insert(v, at, 0, axis=1)
    s2, m2 = np.insert(salts, at, U(12345)), np.insert(msg_salts, at, U(777))
    k2 = np.insert(masks, at, np.uint32(0xFFFFFFFF), axis=1)
    assert v2.shape == (n, R + 4)
    assert np.array_equal(K.row_fingerprints(v2, s2, msg_salts=m2, cv_masks=k2), base)


def test_a_row_of_na_is_zero_and_any_response_is_not():
    R = 9
    salts = rand_salts(7, R)
    assert K.row_fingerprints(np.zeros((4, R), np.uint8), salts).tolist() == [0, 0, 0, 0]
    v = np.zeros((len(CODES) - 1) * R, dtype=np.uint8).reshape(-1, R)
    for k, code in enumerate(CODES[1:]):
        v[k, k % R] = code
    fp = K.row_fingerprints(v, salts)
    assert (fp != 0).all() and np.unique(fp).size == fp.size
    big = matrix(11, 2000, R)
    fp = K.row_fingerprints(big, salts)
    assert np.array_equal(fp == 0, (big == 0).all(axis=1))


def test_one_cell_changes_its_row_only():
    n, R = 257, 18
    v = matrix(21, n, R)
    salts, masks = rand_salts(3, R), rand_masks(8, (n, R))
    base = K.row_fingerprints(v, salts, cv_masks=masks)
    rng = np.random.default_rng(9)
    for _ in range(40):
        i, r = int(rng.integers(n)), int(rng.integers(R))
        w = v.copy()
        w[i, r] = CODES[(np.flatnonzero(CODES == v[i, r])[0] + 1 + int(rng.integers(len(CODES) - 1))) % len(CODES)]
        assert w[i, r] != v[i, r]
        got = K.row_fingerprints(w, salts, cv_masks=masks)
        assert np.flatnonzero(got != base).tolist() == [i]
        assert K.changed_fingerprints(base, got).tolist() == [i]


def test_mask_word_counts_on_fail_cells_with_the_flag_only():
    n, R = 300, 6
    v = matrix(33, n, R)
    salts, masks = rand_salts(4, R), rand_masks(6, (n, R))
    with_m, without = K.row_fingerprints(v, salts, cv_masks=masks), K.row_fingerprints(v, salts)
    fails = np.argwhere(v == FAIL)
    others = np.argwhere((v != FAIL) & (v != 0))
    assert len(fails) > 20 and len(others) > 20
    for i, r in fails[:20]:
        for bit in (0, 31):  # a versioned check, KPE_CVM_XMATCH
            m2 = masks.copy()
            m2[i, r] ^= np.uint32(1 << bit)
            assert np.flatnonzero(K.row_fingerprints(v, salts, cv_masks=m2) != with_m).tolist() == [i]
    assert np.array_equal(K.row_fingerprints(v, salts, cv_masks=None), without)
    # the words of cells that are not FAIL (NA cells too) are ignored
    m2 = masks.copy()
    m2[v != FAIL] = ~m2[v != FAIL]
    assert np.array_equal(K.row_fingerprints(v, salts, cv_masks=m2), with_m)
    # with all-zero words the flag changes nothing
    assert np.array_equal(K.row_fingerprints(v, salts, cv_masks=np.zeros((n, R), np.uint32)), without)


def test_message_salt_changes_exactly_the_rows_with_a_message_cell():
    n, R = 400, 6
    v = matrix(41, n, R)
    salts = rand_salts(5, R)
    base = K.row_fingerprints(v, salts, msg_salts=salts)
    for msg_codes in (K.MESSAGE_CODES, K.SEL(1), K.SEL(FAIL), 0):
        for r in range(R):
            bumped = salts.copy()
            bumped[r] ^= U(1)  # a resourceVersion, an edit counter
            got = K.row_fingerprints(v, salts, msg_salts=bumped, msg_codes=msg_codes)
            want = np.flatnonzero(((msg_codes >> v[:, r].astype(np.uint32)) & 1) != 0)
            assert np.flatnonzero(got != base).tolist() == want.tolist(), (msg_codes, r)
            assert (want.size > 0) == (msg_codes != 0)


def test_rule_salts_are_fnv1a_mix64_of_the_rule_names():
    for pols in ([restricted_latest()], [pss_policy(f"pol-{i}", "baseline" if i % 2 else "restricted") for i in range(200)]):
        ps = K.PolicySet(pols)
        got = K.rule_salts(ps)
        assert got.dtype == np.uint64 and got.shape == (ps.num_rules,)
        assert np.array_equal(got, name_salts(ps.rule_names))
        assert (got != 0).all()
        assert np.unique(got).size == len(set(ps.rule_names)) == ps.num_rules


@pytest.mark.parametrize("n,Ro,Rn", DELTA_SHAPES, ids=[f"n{n}-r{a}-r{b}" for n, a, b in DELTA_SHAPES])
def test_differing_fingerprints_are_the_exact_forms_changed_rows(n, Ro, Rn):
    """Salts by rule name pair the columns the way the column map does: a mapped column shares its
    name, an unmapped one on either side has a fresh name. Seeded inputs: a collision would show
    here."""
    saw_some = False
    for name, cmap in maps(Ro, Rn).items():
        old, new = matrices(n * 31 + Ro * 7 + Rn, n, Ro, Rn, cmap)
        new_names = [f"pol/new-{r}" for r in range(Rn)]
        old_names = [f"pol/old-only-{o}" for o in range(Ro)]
        for r in range(Rn):
            if cmap[r] >= 0:
                old_names[cmap[r]] = new_names[r]
        fo = K.row_fingerprints(old, name_salts(old_names)) if Ro else np.zeros(n, U)
        fn = K.row_fingerprints(new, name_salts(new_names)) if Rn else np.zeros(n, U)
        want, _, total = K.changed_rows(old, new, cmap)
        got = K.changed_fingerprints(fo, fn)
        assert got.dtype == np.uint64 and np.array_equal(got, want), (name, got.size, total)
        assert np.array_equal(got, np.flatnonzero(fo != fn).astype(U))
        saw_some |= total > 0
    if n >= 257:
        assert saw_some


def test_cap_leaves_the_rest_untouched():
    L = load()
    a = K.row_fingerprints(matrix(1, 2000, 3), rand_salts(1, 3))
    b = K.row_fingerprints(matrix(2, 2000, 3), rand_salts(1, 3))
    want = np.flatnonzero(a != b).astype(U)
    total = want.size
    assert 100 < total < 2000
    assert L.kpe_changed_fingerprints_host(a.ctypes.data, b.ctypes.data, 2000, None, 0) == total  # count only
    cap = total // 2
    rows = np.full(total + 8, 0xDEADBEEFDEADBEEF, dtype=U)
    assert L.kpe_changed_fingerprints_host(a.ctypes.data, b.ctypes.data, 2000, rows.ctypes.data, cap) == total
    assert np.array_equal(rows[:cap], want[:cap]) and (rows[cap:] == U(0xDEADBEEFDEADBEEF)).all()
    rows[:] = U(0xDEADBEEFDEADBEEF)
    assert L.kpe_changed_fingerprints_host(a.ctypes.data, b.ctypes.data, 2000, rows.ctypes.data, 1 << 40) == total
    assert np.array_equal(rows[:total], want) and (rows[total:] == U(0xDEADBEEFDEADBEEF)).all()
    assert np.array_equal(K.changed_fingerprints(a, b, cap=cap), want[:cap])
    assert L.kpe_changed_fingerprints_host(a.ctypes.data, b.ctypes.data, 2000, None, 4) == -KPE_E_INVALID
    assert L.kpe_changed_fingerprints_host(None, b.ctypes.data, 2000, None, 0) == -KPE_E_INVALID
    # the twin writes nrows entries and nothing after them
    out = np.full(12, 0xDEADBEEFDEADBEEF, dtype=U)
    v, s = matrix(3, 10, 4), rand_salts(2, 4)
    assert L.kpe_row_fingerprints_host(4, v.ctypes.data, None, 10, s.ctypes.data, None, 0, 0, out.ctypes.data) == 0
    assert np.array_equal(out[:10], spec_fp(v, s)) and (out[10:] == U(0xDEADBEEFDEADBEEF)).all()


def test_host_twin_argument_errors():
    L = load()
    v, s, out = np.zeros((4, 3), np.uint8), rand_salts(1, 3), np.zeros(4, U)
    m = np.zeros((4, 3), np.uint32)
    twin = lambda vv, mm, ss, fl, oo: L.kpe_row_fingerprints_host(3, vv, mm, 4, ss, None, 0, fl, oo)
    assert twin(v.ctypes.data, None, s.ctypes.data, 0, out.ctypes.data) == 0
    assert twin(v.ctypes.data, m.ctypes.data, s.ctypes.data, K.FP_MASKS, out.ctypes.data) == 0
    assert twin(None, None, s.ctypes.data, 0, out.ctypes.data) == KPE_E_INVALID
    assert twin(v.ctypes.data, None, None, 0, out.ctypes.data) == KPE_E_INVALID
    assert twin(v.ctypes.data, None, s.ctypes.data, 0, None) == KPE_E_INVALID
    assert twin(v.ctypes.data, None, s.ctypes.data, K.FP_MASKS, out.ctypes.data) == KPE_E_INVALID  # the flag without words
    assert twin(v.ctypes.data, m.ctypes.data, s.ctypes.data, 2, out.ctypes.data) == KPE_E_INVALID  # an unknown flag
    assert L.kpe_row_fingerprints_host(3, None, None, 0, None, None, 0, 0, None) == 0  # no rows: nothing to read
    assert L.kpe_last_error()
    with pytest.raises(ValueError):
        K.row_fingerprints(v, s[:2])
    with pytest.raises(ValueError):
        K.row_fingerprints(v, None)
    with pytest.raises(ValueError):
        K.changed_fingerprints(out, out[:3])


def test_device_entry_points_check_arguments_before_any_device_call():
    L = load()
    ps = K.PolicySet([restricted_latest()])
    corpus = K.Corpus([{"apiVersion": "v1", "kind": "Pod", "metadata": {"name": "a"}}])  # never uploaded
    R = ps.num_rules
    salts = K.rule_salts(ps)
    out = np.full(4, 0xDEADBEEFDEADBEEF, dtype=U)
    rows = np.full(4, 0xDEADBEEFDEADBEEF, dtype=U)
    vr = np.full((4, R), 0xA5, dtype=np.uint8)
    o, rw = out.ctypes.data, rows.ctypes.data
    # any non-NULL device handle will do: it is never dereferenced by these checks
    fake_dev = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    assert L.kpe_fp_rule_salts(None, o) == KPE_E_INVALID and L.kpe_fp_rule_salts(ps.h, None) == KPE_E_INVALID
    for args in ((None, ps.h, corpus.h), (fake_dev, None, corpus.h), (fake_dev, ps.h, None)):
        assert L.kpe_fetch_row_fingerprints(*args, None, None, 0, 0, 0, 1, o) == KPE_E_INVALID
        assert L.kpe_fingerprints_keep(*args, None, None, 0, 0) == KPE_E_INVALID
        assert L.kpe_changed_rows_fp(*args, None, None, 0, 0, rw, None, None, 4) == -KPE_E_INVALID
    h = (fake_dev, ps.h, corpus.h)
    assert L.kpe_fetch_row_fingerprints(*h, None, None, 0, 0, 0, 1, None) == KPE_E_INVALID  # rows without out
    assert L.kpe_fetch_row_fingerprints(*h, None, None, 0, 2, 0, 1, o) == KPE_E_INVALID  # an unknown flag
    for row0, nrows in ((0, 2), (1, 1), (2, 0), (0, 1 << 63), ((1 << 64) - 1, 2)):  # a window past N = 1
        assert L.kpe_fetch_row_fingerprints(*h, None, None, 0, 0, row0, nrows, o) == KPE_E_INVALID
    assert L.kpe_fetch_row_fingerprints(*h, None, None, 0, 0, 1, 0, None) == 0  # no rows: writes nothing
    assert L.kpe_fetch_row_fingerprints(*h, salts.ctypes.data, None, 0, 0, 0, 1, o) == KPE_E_STATE  # not uploaded
    assert L.kpe_fingerprints_keep(*h, None, None, 0, 2) == KPE_E_INVALID
    assert L.kpe_fingerprints_keep(*h, None, None, 0, 0) == KPE_E_STATE
    assert L.kpe_fingerprints_load(None, corpus.h, o, 1) == KPE_E_INVALID
    assert L.kpe_fingerprints_load(fake_dev, None, o, 1) == KPE_E_INVALID
    assert L.kpe_fingerprints_load(fake_dev, corpus.h, None, 1) == KPE_E_INVALID
    assert L.kpe_fingerprints_load(fake_dev, corpus.h, o, 2) == KPE_E_INVALID  # n != N
    assert L.kpe_fingerprints_load(fake_dev, corpus.h, o, 0) == KPE_E_INVALID
    assert L.kpe_fingerprints_load(fake_dev, corpus.h, o, 1) == KPE_E_STATE  # not uploaded
    assert L.kpe_fingerprints_fetch(None, corpus.h, 0, 1, o) == KPE_E_INVALID
    assert L.kpe_fingerprints_fetch(fake_dev, None, 0, 1, o) == KPE_E_INVALID
    assert L.kpe_fingerprints_fetch(fake_dev, corpus.h, 0, 1, None) == KPE_E_INVALID
    assert L.kpe_fingerprints_fetch(fake_dev, corpus.h, 1, 1, o) == KPE_E_INVALID  # a window past N
    assert L.kpe_fingerprints_fetch(fake_dev, corpus.h, 0, 1, o) == KPE_E_STATE  # nothing kept
    assert L.kpe_fingerprints_drop(None, corpus.h) == KPE_E_INVALID and L.kpe_fingerprints_drop(fake_dev, None) == KPE_E_INVALID
    assert L.kpe_fingerprints_drop(fake_dev, corpus.h) == 0  # nothing kept: nothing to do
    assert L.kpe_fingerprints_kept(corpus.h) == 0 and L.kpe_fingerprints_kept(None) == 0
    assert L.kpe_changed_rows_fp(*h, None, None, 0, 0, None, None, None, 4) == -KPE_E_INVALID  # cap without rows
    assert L.kpe_changed_rows_fp(*h, None, None, 0, 2, rw, None, None, 4) == -KPE_E_INVALID
    assert L.kpe_changed_rows_fp(*h, None, None, 0, 0, rw, vr.ctypes.data, o, 4) == -KPE_E_STATE  # nothing kept
    assert L.kpe_changed_rows_fp(*h, None, None, 0, 0, None, None, None, 0) == -KPE_E_STATE
    assert L.kpe_last_error()
    # no refused call wrote anything
    assert (out == U(0xDEADBEEFDEADBEEF)).all() and (rows == U(0xDEADBEEFDEADBEEF)).all() and (vr == 0xA5).all()


def test_more_rules_than_the_kernel_takes_is_a_limit():
    """KPE_DELTA_MAX_RULES = 4096: a row fits the kernel's tile. Checked before the state and before
    any device call; the host twin has no such limit."""
    L = load()
    ps = K.PolicySet([pss_policy(f"p{i}", "baseline") for i in range(1366)])  # three rules each after autogen
    R = ps.num_rules
    assert R == 4098
    corpus = K.Corpus([{"apiVersion": "v1", "kind": "Pod", "metadata": {"name": "a"}}])
    fake_dev = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    out = np.zeros(1, U)
    assert L.kpe_fetch_row_fingerprints(fake_dev, ps.h, corpus.h, None, None, 0, 0, 0, 1, out.ctypes.data) == KPE_E_LIMIT
    assert L.kpe_fingerprints_keep(fake_dev, ps.h, corpus.h, None, None, 0, 0) == KPE_E_LIMIT
    assert L.kpe_changed_rows_fp(fake_dev, ps.h, corpus.h, None, None, 0, 0, None, None, None, 0) == -KPE_E_LIMIT
    v = np.zeros((3, R), np.uint8)
    v[1, R - 1] = 2
    salts = K.rule_salts(ps)
    fp = K.row_fingerprints(v, salts)
    assert np.array_equal(fp, spec_fp(v, salts)) and np.flatnonzero(fp).tolist() == [1]


# ---- the kernel's body on the host ------------------------------------------------------------
# (R, n): the rule counts and sizes of tests/test_gpu_fp.py, the group edges (4096 / R rows), rows
# longer than a 16-byte load, the widest row the kernel takes (one row per group)
HARNESS_SHAPES = ([(1, n) for n in (1, 15, 16, 17, 1025, 4097)] + [(3, n) for n in (1, 5, 6, 1365, 1366, 5000)] +
                  [(R, n) for R in (15, 16, 18) for n in (227, 4096)] + [(204, n) for n in (21, 2000, 20100)] +
                  [(4096, 5)])


@pytest.fixture(scope="module")
def fp_check():
    return build_host_tool("fp_check")


@pytest.mark.parametrize("R,n", HARNESS_SHAPES, ids=[f"r{r}-n{n}" for r, n in HARNESS_SHAPES])
def test_kernel_body_under_asan_matches_the_twin(fp_check, tmp_path, R, n):
    v = matrix(n + R, n, R)
    salts, msg_salts = rand_salts(n, R), rand_salts(n + 1, R)
    masks = rand_masks(n + 2, (n, R))
    grid = 3 if n < 20000 else 7  # fewer blocks than groups: the persistent loop
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1")
    case, outp = tmp_path / "case.bin", tmp_path / "fp.bin"
    for with_masks in (False, True):
        want = K.row_fingerprints(v, salts, msg_salts=msg_salts, cv_masks=masks if with_masks else None)
        assert np.array_equal(want, spec_fp(v, salts, msg_salts, K.MESSAGE_CODES, masks if with_masks else None))
        for row0 in (0, 1, 37):
            if row0 > n:
                continue
            nrows = n - row0
            with open(case, "wb") as f:
                f.write(struct.pack("<QIIIIQQ", n, R, grid, 1 if with_masks else 0, K.MESSAGE_CODES, row0, nrows))
                f.write(salts.tobytes() + msg_salts.tobytes() + v.tobytes())
                if with_masks:
                    f.write(masks.tobytes())
            res = subprocess.run([fp_check, str(case), str(outp)], env=env, capture_output=True, text=True)
            assert res.returncode == 0, res.stdout + res.stderr
            got = np.fromfile(outp, dtype=U)
            assert np.array_equal(got, want[row0:]), (with_masks, row0, res.stdout)
    if n >= 227:
        assert (want != 0).any() and ((want == 0).any() or R > 8)
