"""Result deltas, host half (no GPU): the entry points are exported, the host twins
(kpe_changed_rows_host, kpe_delta_transitions_host) agree with the rule of include/kpe.h stated in
numpy, `cap` leaves the rest of the buffers alone, the column map pairs rules by name, the argument
checks of the device entry points come before any device call, and the flag pass of the kernel
(kyverno_amd/csrc/delta.inl) run lane by lane on the host under ASan / UBSan
(scripts/delta_check.cpp) gives the twin's rows at every shape the GPU suite uses."""
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

CODES = np.array([0, 1, 2, 3, 4, 5, 7], dtype=np.uint8)  # the kpe_verdict alphabet
KPE_E_INVALID, KPE_E_LIMIT, KPE_E_STATE = 1, 4, 5


def spec_changed(old, new, cmap, always):
    """Row i is changed iff a new cell differs from its partner (the kept cell the map names, NA
    without one), or a new cell's verdict is in its column's `always` mask, or a kept column no
    entry names holds a response."""
    n, Rn = new.shape
    Ro = old.shape[1]
    partner = np.zeros((n, Rn), dtype=np.uint8)
    for r in range(Rn):
        if cmap[r] >= 0:
            partner[:, r] = old[:, cmap[r]]
    ch = (new != partner).any(axis=1)
    ch |= (((always[None, :].astype(np.uint32) >> new.astype(np.uint32)) & 1) != 0).any(axis=1)
    gone = [o for o in range(Ro) if o not in set(int(x) for x in cmap)]
    ch |= (old[:, gone] != 0).any(axis=1)
    return np.flatnonzero(ch).astype(np.uint64)


def spec_transitions(old, new, cmap):
    n, Rn = new.shape
    out = np.zeros((Rn, 8, 8), dtype=np.uint64)
    for r in range(Rn):
        o = old[:, cmap[r]] if cmap[r] >= 0 else np.zeros(n, dtype=np.uint8)
        np.add.at(out[r], (o.astype(np.int64), new[:, r].astype(np.int64)), 1)
    return out


def matrices(seed, n, Ro, Rn, cmap, p=0.02):
    """A seeded kept matrix over the alphabet, mostly NA like a real one, and a new matrix that is
    its image under the map with a fraction p of the cells redrawn."""
    rng = np.random.default_rng(seed)
    old = rng.choice(CODES, size=(n, Ro), p=[0.7, 0.1, 0.1, 0.02, 0.03, 0.03, 0.02]).astype(np.uint8)
    new = np.zeros((n, Rn), dtype=np.uint8)
    for r in range(Rn):
        if cmap[r] >= 0:
            new[:, r] = old[:, cmap[r]]
    hit = rng.random((n, Rn)) < p
    new[hit] = rng.choice(CODES, size=int(hit.sum()))
    return old, new


def maps(Ro, Rn, seed=1):
    """identity (as far as it goes), reversed, entries of -1, kept columns left unmapped"""
    rng = np.random.default_rng(seed)
    k = min(Ro, Rn)
    ident = np.full(Rn, -1, dtype=np.int32)
    ident[:k] = np.arange(k)
    rev = np.full(Rn, -1, dtype=np.int32)
    rev[:k] = np.arange(Ro - 1, Ro - 1 - k, -1)
    holes = ident.copy()
    holes[::2] = -1
    perm = np.full(Rn, -1, dtype=np.int32)
    perm[:k] = rng.permutation(Ro)[:k]
    return {"identity": ident, "reversed": rev, "holes": holes, "perm": perm, "none": np.full(Rn, -1, dtype=np.int32)}


SHAPES = [(0, 3, 3), (1, 1, 1), (17, 1, 1), (300, 3, 3), (300, 3, 6), (300, 6, 3), (257, 18, 15), (64, 204, 204),
          (50, 1, 7), (50, 7, 1)]


def test_symbols_exported():
    L = load()
    for name in ("kpe_results_keep", "kpe_results_drop", "kpe_results_kept_rules", "kpe_results_kept_rule_name",
                 "kpe_delta_column_map", "kpe_changed_rows", "kpe_delta_transitions", "kpe_changed_rows_host",
                 "kpe_delta_transitions_host"):
        assert hasattr(L, name), name
    for name in ("changed_rows", "delta_transitions", "column_map", "ResidentScanner"):
        assert callable(getattr(K, name)), name
    for name in ("keep_results", "changed_rows", "delta_transitions"):
        assert callable(getattr(K.Engine, name)), name


@pytest.mark.parametrize("n,Ro,Rn", SHAPES, ids=[f"n{n}-r{a}-r{b}" for n, a, b in SHAPES])
def test_host_twins_match_the_rule(n, Ro, Rn):
    saw_some, saw_not_all = False, False
    for name, cmap in maps(Ro, Rn).items():
        old, new = matrices(n * 31 + Ro * 7 + Rn, n, Ro, Rn, cmap)
        for always in (np.zeros(Rn, np.uint8), np.where(np.arange(Rn) % 2 == 1, K.SEL(2), 0).astype(np.uint8)):
            want = spec_changed(old, new, cmap, always)
            rows, vr, total = K.changed_rows(old, new, cmap, always)
            assert rows.dtype == np.uint64 and vr.dtype == np.uint8 and vr.shape == (want.size, Rn)
            assert total == want.size and np.array_equal(rows, want), (name, total, want.size)
            assert np.array_equal(vr, new[want.astype(np.int64)]), name
            saw_some |= 0 < total
            saw_not_all |= total < n
        got = K.delta_transitions(old, new, cmap)
        assert got.shape == (Rn, 8, 8) and got.dtype == np.uint64
        assert np.array_equal(got, spec_transitions(old, new, cmap)), name
        assert (got.reshape(Rn, 64).sum(axis=1) == n).all()  # every row lands once per column
    if n >= 257:
        assert saw_some and saw_not_all


def test_every_always_bit_on_its_own():
    n, R = 70, 4
    ident = np.arange(R, dtype=np.int32)
    old = np.repeat(np.tile(CODES, n // len(CODES))[:, None], R, axis=1)  # every code, equal matrices
    assert K.changed_rows(old, old, ident)[2] == 0
    for bit in range(8):
        for col in range(R):
            always = np.zeros(R, np.uint8)
            always[col] = 1 << bit
            rows, _, total = K.changed_rows(old, old, ident, always)
            want = spec_changed(old, old, ident, always)
            assert np.array_equal(rows, want) and total == want.size
            assert np.array_equal(rows, np.flatnonzero(old[:, col] == bit).astype(np.uint64))  # 6: no such code
    # a scalar mask is broadcast to every rule
    assert K.changed_rows(old, old, ident, K.SEL(2))[2] == int((old[:, 0] == 2).sum())


def test_equal_matrices_give_a_diagonal_table():
    ident = np.arange(5, dtype=np.int32)
    old, _ = matrices(9, 400, 5, 5, ident)
    t = K.delta_transitions(old, old, ident)
    off = t.copy()
    off[:, np.arange(8), np.arange(8)] = 0
    assert not off.any() and (t.reshape(5, 64).sum(axis=1) == 400).all()
    for r in range(5):
        assert np.array_equal(np.diagonal(t[r]), np.bincount(old[:, r], minlength=8).astype(np.uint64))
    # an unmapped column's old code is NA: the table has one row
    t = K.delta_transitions(old, old, np.full(5, -1, dtype=np.int32))
    assert not t[:, 1:, :].any() and (t[:, 0, :].sum(axis=1) == 400).all()


def test_cap_leaves_the_rest_untouched():
    L = load()
    cmap = maps(6, 3)["perm"]
    old, new = matrices(5, 2000, 6, 3, cmap)
    always = np.zeros(3, np.uint8)
    want = spec_changed(old, new, cmap, always)
    total = want.size
    assert 100 < total < 2000
    args = (old.ctypes.data, new.ctypes.data, 2000, 6, 3, cmap.ctypes.data, always.ctypes.data)
    assert L.kpe_changed_rows_host(*args, None, None, 0) == total  # count only
    assert L.kpe_changed_rows_host(*args[:6], None, None, None, 0) == total  # always == NULL: all zero
    cap = total // 2
    rows = np.full(total + 8, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    vr = np.full((total + 8, 3), 0xA5, dtype=np.uint8)
    assert L.kpe_changed_rows_host(*args, rows.ctypes.data, vr.ctypes.data, cap) == total
    assert np.array_equal(rows[:cap], want[:cap]) and np.array_equal(vr[:cap], new[want[:cap].astype(np.int64)])
    assert (rows[cap:] == np.uint64(0xDEADBEEFDEADBEEF)).all() and (vr[cap:] == 0xA5).all()
    rows[:] = np.uint64(0xDEADBEEFDEADBEEF)
    assert L.kpe_changed_rows_host(*args, rows.ctypes.data, None, 1 << 40) == total
    assert np.array_equal(rows[:total], want) and (rows[total:] == np.uint64(0xDEADBEEFDEADBEEF)).all()
    r2, v2, t2 = K.changed_rows(old, new, cmap, cap=cap)
    assert t2 == total and np.array_equal(r2, want[:cap]) and v2.shape == (cap, 3)
    assert K.changed_rows(old, new, cmap, with_verdicts=False)[1].shape == (0, 3)


def test_column_map_pairs_rules_by_name():
    old = ["a/x", "a/y", "b/x", "c/x"]
    assert K.column_map(old, old).tolist() == [0, 1, 2, 3]
    assert K.column_map(old, ["c/x", "b/x", "a/y", "a/x"]).tolist() == [3, 2, 1, 0]  # reordered
    assert K.column_map(old, ["new/x"] + old).tolist() == [-1, 0, 1, 2, 3]  # an added name
    assert K.column_map(old, ["a/x", "b/x", "c/x"]).tolist() == [0, 2, 3]  # a removed one: column 1 unmapped
    assert K.column_map(old, []).dtype == np.int32 and K.column_map([], ["a/x"]).tolist() == [-1]
    for o, nw in ((old + ["a/x"], old), (old, ["a/x", "a/x"])):
        with pytest.raises(K.KpeError) as e:
            K.column_map(o, nw)
        assert e.value.status == KPE_E_INVALID


def test_host_twin_argument_errors():
    L = load()
    old = np.zeros((4, 3), np.uint8)
    new = np.zeros((4, 2), np.uint8)
    out = np.zeros((2, 64), np.uint64)
    rows = np.zeros(4, np.uint64)

    def changed(cmap, o=old, nw=new, rows_p=rows.ctypes.data, cap=4):
        m = np.asarray(cmap, dtype=np.int32)
        return L.kpe_changed_rows_host(None if o is None else o.ctypes.data, None if nw is None else nw.ctypes.data, 4,
                                       3, 2, m.ctypes.data, None, rows_p, None, cap)

    assert changed([0, 1]) == 0
    assert changed([0, 3]) == -KPE_E_INVALID  # an entry >= Ro
    assert changed([0, -2]) == -KPE_E_INVALID
    assert changed([1, 1]) == -KPE_E_INVALID  # a kept column named twice
    assert changed([0, 1], rows_p=None) == -KPE_E_INVALID  # cap > 0 without rows
    assert changed([0, 1], o=None) == -KPE_E_INVALID and changed([0, 1], nw=None) == -KPE_E_INVALID
    assert L.kpe_changed_rows_host(old.ctypes.data, new.ctypes.data, 4, 3, 2, None, None, None, None, 0) == -KPE_E_INVALID
    for m in ([0, 3], [1, 1]):
        mm = np.asarray(m, dtype=np.int32)
        assert L.kpe_delta_transitions_host(old.ctypes.data, new.ctypes.data, 4, 3, 2, mm.ctypes.data,
                                            out.ctypes.data) == KPE_E_INVALID
    mm = np.asarray([0, 1], dtype=np.int32)
    assert L.kpe_delta_transitions_host(old.ctypes.data, new.ctypes.data, 4, 3, 2, mm.ctypes.data, None) == KPE_E_INVALID
    assert L.kpe_last_error()
    with pytest.raises(ValueError):
        K.changed_rows(old, new, [0, 1, 2])
    with pytest.raises(ValueError):
        K.changed_rows(old, np.zeros((5, 2), np.uint8), [0, 1])


def test_device_entry_points_check_arguments_before_any_device_call():
    L = load()
    ps = K.PolicySet([restricted_latest()])
    corpus = K.Corpus([{"apiVersion": "v1", "kind": "Pod", "metadata": {"name": "a"}}])  # never uploaded
    R = ps.num_rules
    rows = (ctypes.c_uint64 * 4)()
    out = (ctypes.c_uint64 * (64 * R))()
    cmap = (ctypes.c_int32 * R)(*range(R))
    # any non-NULL device handle will do: it is never dereferenced by these checks
    fake_dev = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    assert L.kpe_results_keep(None, ps.h, corpus.h) == KPE_E_INVALID
    assert L.kpe_results_keep(fake_dev, None, corpus.h) == KPE_E_INVALID
    assert L.kpe_results_keep(fake_dev, ps.h, None) == KPE_E_INVALID
    assert L.kpe_results_keep(fake_dev, ps.h, corpus.h) == KPE_E_STATE  # not uploaded: no evaluation
    assert L.kpe_results_drop(None, corpus.h) == KPE_E_INVALID and L.kpe_results_drop(fake_dev, None) == KPE_E_INVALID
    assert L.kpe_results_drop(fake_dev, corpus.h) == 0  # nothing kept: nothing to do
    assert L.kpe_results_kept_rules(corpus.h) == -1 and L.kpe_results_kept_rules(None) == -1
    assert L.kpe_results_kept_rule_name(corpus.h, 0) is None
    assert L.kpe_delta_column_map(None, ps.h, cmap) == KPE_E_INVALID
    assert L.kpe_delta_column_map(corpus.h, None, cmap) == KPE_E_INVALID
    assert L.kpe_delta_column_map(corpus.h, ps.h, cmap) == KPE_E_STATE  # nothing kept
    for args in ((None, ps.h, corpus.h), (fake_dev, None, corpus.h), (fake_dev, ps.h, None)):
        assert L.kpe_changed_rows(*args, cmap, None, rows, None, 4) == -KPE_E_INVALID
        assert L.kpe_delta_transitions(*args, cmap, out) == KPE_E_INVALID
    assert L.kpe_changed_rows(fake_dev, ps.h, corpus.h, cmap, None, None, None, 4) == -KPE_E_INVALID  # cap without rows
    assert L.kpe_delta_transitions(fake_dev, ps.h, corpus.h, cmap, None) == KPE_E_INVALID
    assert L.kpe_changed_rows(fake_dev, ps.h, corpus.h, cmap, None, rows, None, 4) == -KPE_E_STATE  # nothing kept
    assert L.kpe_delta_transitions(fake_dev, ps.h, corpus.h, cmap, out) == KPE_E_STATE
    assert L.kpe_last_error()


def test_more_rules_than_the_kernel_stages_is_a_limit():
    """KPE_DELTA_MAX_RULES = 4096 a side: the kept rows of a group and the per-rule tables live in
    LDS. Checked before the state and before any device call; the host twins have no such limit."""
    L = load()
    ps = K.PolicySet([pss_policy(f"p{i}", "baseline") for i in range(1366)])  # three rules each after autogen
    R = ps.num_rules
    assert R == 4098
    corpus = K.Corpus([{"apiVersion": "v1", "kind": "Pod", "metadata": {"name": "a"}}])
    fake_dev = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    out = np.zeros((R, 64), np.uint64)
    assert L.kpe_changed_rows(fake_dev, ps.h, corpus.h, None, None, None, None, 0) == -KPE_E_LIMIT
    assert L.kpe_delta_transitions(fake_dev, ps.h, corpus.h, None, out.ctypes.data) == KPE_E_LIMIT
    v = np.zeros((3, R), np.uint8)
    v[1, R - 1] = 2
    ident = np.arange(R, dtype=np.int32)
    assert K.changed_rows(np.zeros_like(v), v, ident)[0].tolist() == [1]


# ---- the kernel's flag pass on the host -------------------------------------------------------
# (Ro, Rn, n): the program pairs and sizes of tests/test_gpu_delta.py
HARNESS_SHAPES = ([(1, 1, n) for n in (1, 15, 16, 17, 1023, 1024, 1025, 4097)] +
                  [(3, 3, n) for n in (1, 5, 6, 64, 1365, 1366, 5000)] +
                  [(3, 6, n) for n in (64, 682, 683, 5000)] + [(6, 3, n) for n in (64, 682, 683, 5000)] +
                  [(18, 15, n) for n in (227, 228, 4096)] +
                  [(204, 204, n) for n in (21, 2000, 20100, 45000)] +
                  # rows longer than a 16-byte load and the widest the kernel takes (one row per group)
                  [(4096, 4095, 5), (37, 4096, 9), (0, 3, 40), (3, 0, 40)])


@pytest.fixture(scope="module")
def delta_check():
    return build_host_tool("delta_check")


@pytest.mark.parametrize("Ro,Rn,n", HARNESS_SHAPES, ids=[f"r{a}-r{b}-n{n}" for a, b, n in HARNESS_SHAPES])
def test_flag_pass_under_asan_matches_the_twin(delta_check, tmp_path, Ro, Rn, n):
    mp = maps(Ro, Rn, seed=n)
    cmap = mp["perm"] if Ro != Rn else (mp["identity"] if n % 2 else mp["holes"])
    if (Ro, Rn) == (3, 6):  # the shape of an added policy: the kept columns shifted by three
        cmap = np.array([-1, -1, -1, 0, 1, 2], dtype=np.int32)
    if (Ro, Rn) == (6, 3):
        cmap = np.array([3, 4, 5], dtype=np.int32)
    wide = Ro > 100 and Rn > 100  # few edits, or every row of a wide matrix is changed
    if wide:
        cmap = mp["identity"].copy()
        cmap[5] = -1  # one rule replaced: its kept column is swept, its new column compared with NA
    old, new = matrices(n + Ro, n, Ro, Rn, cmap, p=0.001 if wide else 0.02)
    always = np.where(np.arange(Rn) % 2 == 1, K.SEL(2), 0).astype(np.uint8)
    if wide:
        always[3:] = 0
    case, flags = tmp_path / "case.bin", tmp_path / "flags.bin"
    grid = 3 if n < 20000 else 7  # fewer blocks than groups: the persistent loop
    with open(case, "wb") as f:
        f.write(struct.pack("<QIIII", n, Ro, Rn, grid, 0))
        f.write(cmap.tobytes() + always.tobytes() + old.tobytes() + new.tobytes())
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([delta_check, str(case), str(flags)], env=env, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    got = np.flatnonzero(np.fromfile(flags, dtype=np.uint8)).astype(np.uint64)
    rows, _, total = K.changed_rows(old, new, cmap, always)
    assert np.array_equal(got, rows), res.stdout
    assert np.array_equal(rows, spec_changed(old, new, cmap, always))
    if n >= 683 and Ro and Rn:
        assert 0 < total < n
