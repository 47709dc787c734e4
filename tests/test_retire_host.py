"""Retired rows and the comparison across corpora, host half (no GPU): the entry points are
exported, kpe_corpus_retire_rows on a corpus that is not uploaded records the set on the host
(union, ascending, unique; a bad row leaves it untouched), and the argument checks of
kpe_changed_pairs / kpe_changed_pairs_fp come before any device call."""
import ctypes

import numpy as np

import kyverno_amd as K
from kyverno_amd._lib import load
from tests.policies import restricted_latest

KPE_E_INVALID, KPE_E_STATE = 1, 5


def u64(*xs):
    return np.array(xs, dtype=np.uint64)


def retired(corpus):
    L = load()
    n = L.kpe_corpus_retired_rows(corpus.h, None, 0)
    out = np.zeros(max(n, 1), dtype=np.uint64)
    assert L.kpe_corpus_retired_rows(corpus.h, out.ctypes.data, n) == n
    return [int(x) for x in out[:n]]


def test_symbols_resolve():
    L = load()
    for name in ("kpe_corpus_retire_rows", "kpe_corpus_retired_rows", "kpe_changed_pairs", "kpe_changed_pairs_fp"):
        assert getattr(L, name) is not None


def test_retire_on_host_corpus():
    L = load()
    corpus = K.Corpus(K.synth_resources(7, 40, mix=2))
    N = corpus.n
    assert retired(corpus) == []
    a = u64(9, 3, 3, 1)  # descending, with a duplicate
    assert L.kpe_corpus_retire_rows(None, corpus.h, a.ctypes.data, a.size) == 0
    assert retired(corpus) == [1, 3, 9]
    b = u64(N - 1, 9, 0, 5, 5)
    assert L.kpe_corpus_retire_rows(None, corpus.h, b.ctypes.data, b.size) == 0
    assert retired(corpus) == [0, 1, 3, 5, 9, N - 1]
    # a row equal to N: refused, the set untouched (the good rows before it included)
    c = u64(2, N)
    assert L.kpe_corpus_retire_rows(None, corpus.h, c.ctypes.data, c.size) == KPE_E_INVALID
    assert retired(corpus) == [0, 1, 3, 5, 9, N - 1]
    # n == 0 is fine, with or without a pointer; a null list with n > 0 is not
    assert L.kpe_corpus_retire_rows(None, corpus.h, None, 0) == 0
    assert L.kpe_corpus_retire_rows(None, corpus.h, c.ctypes.data, 0) == 0
    assert L.kpe_corpus_retire_rows(None, corpus.h, None, 2) == KPE_E_INVALID
    assert L.kpe_corpus_retire_rows(None, None, c.ctypes.data, 1) == KPE_E_INVALID
    assert retired(corpus) == [0, 1, 3, 5, 9, N - 1]
    # cap: the first min(total, cap) entries, the total returned; nothing past cap written
    out = np.full(4, 77, dtype=np.uint64)
    assert L.kpe_corpus_retired_rows(corpus.h, out.ctypes.data, 2) == 6
    assert out.tolist() == [0, 1, 77, 77]
    assert L.kpe_corpus_retired_rows(corpus.h, None, 2) == -KPE_E_INVALID
    assert L.kpe_corpus_retired_rows(None, None, 0) == -KPE_E_INVALID
    # the Python surface, on a corpus that is not uploaded (no device is touched)
    eng = K.Engine.__new__(K.Engine)
    eng.device = None
    eng.retire_rows(corpus, [7, 7, 2])
    assert eng.retired_rows(corpus).tolist() == [0, 1, 2, 3, 5, 7, 9, N - 1]


def test_changed_pairs_argument_checks():
    L = load()
    ps = K.PolicySet([restricted_latest()])
    R = ps.num_rules
    new, old = K.Corpus(K.synth_resources(3, 16)), K.Corpus(K.synth_resources(4, 24))
    fake_dev = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    pairs = u64(0, 0, 15, 23)
    idx = np.zeros(4, dtype=np.uint64)
    cmap = np.arange(R, dtype=np.int32)

    def cp(dev=fake_dev, prog=ps.h, cn=new.h, co=old.h, p=pairs.ctypes.data, n=2, changed=idx.ctypes.data, cap=2):
        return L.kpe_changed_pairs(dev, prog, cn, co, p, n, cmap.ctypes.data, None, changed, None, cap)

    def cpf(dev=fake_dev, prog=ps.h, cn=new.h, co=old.h, p=pairs.ctypes.data, n=2, changed=idx.ctypes.data, cap=2, flags=0):
        return L.kpe_changed_pairs_fp(dev, prog, cn, co, p, n, None, None, 0, flags, changed, None, None, cap)

    for f in (cp, cpf):
        assert f(dev=None) == -KPE_E_INVALID
        assert f(prog=None) == -KPE_E_INVALID
        assert f(cn=None) == -KPE_E_INVALID
        assert f(co=None) == -KPE_E_INVALID
        assert f(p=None) == -KPE_E_INVALID  # npairs > 0 without pairs
        assert f(changed=None) == -KPE_E_INVALID  # cap > 0 without changed
        bad_new, bad_old = u64(16, 0), u64(0, 24)  # a row equal to its corpus's N
        assert f(p=bad_new.ctypes.data, n=1) == -KPE_E_INVALID
        assert f(p=bad_old.ctypes.data, n=1) == -KPE_E_INVALID
        # well-formed arguments: the old corpus keeps nothing (it is not even uploaded)
        assert f() == -KPE_E_STATE
        assert f(p=None, n=0, changed=None, cap=0) == -KPE_E_STATE
    assert cpf(flags=2) == -KPE_E_INVALID  # an unknown fingerprint flag
