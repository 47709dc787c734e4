"""The pattern-leaf table (tests/leaf_cases.py) on the device, in both forms a leaf is decided in:
a bit of the binding's leaf table (kpe_leaf_table_kernel runs pat_leaf_eval once per interned
scalar; at most KPE_LTAB_SLOTS = 256 distinct leaves have a slot) and pat_leaf_eval inside the
walk (the 257th distinct leaf onward). Same expectations as tests/test_leaf_host.py: the oracle
on every cell, the reference's `want` on its own vectors, no undecided cell; and the two forms
agree cell for cell."""
import numpy as np
import pytest

import kyverno_amd as K
from tests import leaf_cases as L

SLOTS = 256  # schema.h KPE_LTAB_SLOTS


@pytest.fixture(scope="module")
def tab():
    pats, vals, want, _, _ = L.table()
    return pats, vals, want, L.ndjson(vals)


@pytest.fixture(scope="module")
def ref(tab, oracle):
    pats, vals, _, nd = tab
    r = oracle.validate(L.policies(pats), nd, nthreads=8)
    assert r.shape == (len(vals), len(pats)) and set(np.unique(r)) <= {1, 2}
    return r


def evaluate(pols, nd):
    v, _, _ = K.Engine(ordinal=0).evaluate(K.PolicySet(pols), K.Corpus(nd))
    return v


@pytest.fixture(scope="module")
def table_form(tab):
    """One program per 256 patterns: every leaf has a slot (one leaf per policy, none with
    variables), so the pattern kernel's leaf-table instance runs and no leaf is evaluated in the walk."""
    pats, _, _, nd = tab
    return np.concatenate([evaluate(L.policies(pats[g:g + SLOTS], first=g), nd) for g in range(0, len(pats), SLOTS)], axis=1)


@pytest.fixture(scope="module")
def walk_form(tab):
    """All patterns in one program, in list order and reversed: the first 256 distinct leaves take the
    slots, the others are decided in the walk. Returns both matrices in list order and, per column,
    the runs in which its leaf was past the slots."""
    pats, _, _, nd = tab
    assert len(pats) > 2 * SLOTS
    fwd = evaluate(L.policies(pats), nd)
    rev = evaluate(L.policies(pats)[::-1], nd)[:, ::-1]
    return fwd, rev


def check(v, ref, tab):
    pats, vals, want, _ = tab
    assert v.shape == ref.shape
    assert not (v == 7).any() and not (v == 6).any()
    bad = np.argwhere(v != ref)
    assert bad.size == 0, f"{len(bad)} cells differ from the oracle, first " \
                          f"{[(vals[i], pats[j], int(v[i, j]), int(ref[i, j])) for i, j in bad[:8]]}"
    wrong = [(name, pats[j], vals[i], w, int(v[i, j])) for (j, i), (name, w) in want.items() if v[i, j] != (1 if w else 2)]
    assert not wrong, wrong[:8]


@pytest.mark.gpu
def test_leaf_table_form(tab, ref, table_form):
    check(table_form, ref, tab)


@pytest.mark.gpu
def test_leaf_walk_form(tab, ref, walk_form):
    fwd, rev = walk_form
    check(fwd, ref, tab)
    check(rev, ref, tab)


@pytest.mark.gpu
def test_leaf_forms_agree(tab, table_form, walk_form):
    """Every leaf is past the 256 slots in the forward run or in the reversed one (the distinct
    leaves of the table are more than twice the slots), so each column compares a table bit with the
    walk's own evaluation."""
    fwd, rev = walk_form
    n = table_form.shape[1]
    in_walk_fwd, in_walk_rev = np.arange(n) >= SLOTS, np.arange(n) < n - SLOTS
    assert (in_walk_fwd | in_walk_rev).all()
    assert np.array_equal(table_form[:, in_walk_fwd], fwd[:, in_walk_fwd])
    assert np.array_equal(table_form[:, in_walk_rev], rev[:, in_walk_rev])
    assert np.array_equal(fwd, rev)


@pytest.mark.gpu
@pytest.mark.parametrize("nscal", L.SCALAR_COUNTS)
def test_leaf_table_scalar_tail(oracle, nscal):
    """The leaf table's two-word ballot store and ltab_words at 7, 63, 64, 65, 127 and 129 interned
    scalars: a truncated document list whose scalar count is derived in leaf_cases.scalar_count
    (three fixed entries, three envelope strings, one per distinct value) and confirmed against the
    flattener by tests/test_leaf_host.py. 7 is the smallest corpus of these documents."""
    vals = L.simple_head(nscal - 7) + ["7777"]  # the last scalar is a number the `>` forms pass
    assert L.scalar_count(vals) == nscal
    pats = L.patterns()[1::3][:SLOTS]  # the `>` and `<=` forms: both verdicts on these values
    pols, nd = L.policies(pats), L.ndjson(vals)
    v, r = evaluate(pols, nd), oracle.validate(pols, nd)
    assert np.array_equal(v, r)
    assert (r == 1).any() and (r == 2).any()
    assert (r[-1] == 1).any()  # the last scalar's bit is read as set somewhere


@pytest.mark.gpu
def test_leaf_text_alignment(oracle):
    """The last scalar text at each of the 8 byte alignments, ending the text buffer (8-byte loads
    read into the slack behind it), with the longest and the shortest string last; table form and,
    with more than 256 leaves in the program, the walk."""
    globs = [p for p in L.patterns() if any(c in p for c in "*?") or not p.isascii()]
    assert len(globs) <= SLOTS
    many = L.patterns()[:SLOTS] + globs  # the globs are past the slots here
    for pats in (globs, many):
        ps = K.PolicySet(L.policies(pats))
        eng = K.Engine(ordinal=0)
        for vals in L.aligned_tails():
            nd = L.ndjson(vals)
            v, _, _ = eng.evaluate(ps, K.Corpus(nd))
            r = oracle.validate(L.policies(pats), nd)
            assert np.array_equal(v, r), vals[-2:]
            assert (r[-1] == 1).any() and (r[-1] == 2).any()
