"""go-jmespath builtins (contains, starts_with, ends_with, not_null, values() / keys() in function
form) evaluated by kpe_cond_kernel: bit-exact verdict matrices against the oracle on synthetic
corpora (4096 rows: 64 full waves) with the edge documents of tests/jmespath_func_cases.py riding
in a partial wave. The host build of the same VM text is tests/test_jmespath_funcs.py."""
import json

import numpy as np
import pytest

import kyverno_amd as K
from tests import jmespath_func_cases as J

pytestmark = pytest.mark.gpu


def _nd(seed, mix):
    return K.synth_resources(seed, 4096, mix=mix).rstrip(b"\n") + b"\n" + J.edge_ndjson()


def _assert_equal(v, ref, names):
    assert v.shape == ref.shape
    bad = np.argwhere(v != ref)
    assert bad.size == 0, f"{len(bad)} mismatching cells, first {[(int(i), names[j]) for i, j in bad[:5]]} " \
                          f"gpu={[int(v[i, j]) for i, j in bad[:5]]} ref={[int(ref[i, j]) for i, j in bad[:5]]}"


@pytest.mark.parametrize("mix,seed", [(1, 0xF3), (2, 0xF4)])
def test_functions_bit_exact(oracle, mix, seed):
    pols = J.func_policy_set()
    nd = _nd(seed, mix)
    ps = K.PolicySet(pols)
    v, _, cnt = K.Engine(ordinal=0).evaluate(ps, K.Corpus(nd))
    ref = oracle.validate(pols, nd, nthreads=8)
    assert v.shape[0] == 4096 + len(J.edge_documents())
    assert (v == 7).sum() == 0 and (v == 6).sum() == 0
    _assert_equal(v, ref, ps.rule_names)
    for r in range(v.shape[1]):
        col = v[:, r]
        assert len(set(np.unique(col).tolist()) - {0}) >= 2, ps.rule_names[r]
        assert cnt[r]["pass"] == int((col == 1).sum()) and cnt[r]["fail"] == int((col == 2).sum())
        assert cnt[r]["error"] == int((col == 4).sum()) and cnt[r]["skip"] == int((col == 5).sum())
        assert cnt[r]["undecided"] == 0


def test_list_needle_is_undecided(oracle):
    pols = J.needle_list_policy()
    nd = _nd(0xF5, 2)
    deep = np.array(J.needle_list_rows([json.loads(l) for l in nd.split(b"\n") if l]))
    v, _, cnt = K.Engine(ordinal=0).evaluate(K.PolicySet(pols), K.Corpus(nd))
    ref = oracle.validate(pols, nd, nthreads=8)
    applies = ref[:, 0] != 0
    assert 0 < (deep & applies).sum() < applies.sum()
    assert (v[deep & applies, 0] == 7).all()
    assert (v == 7).sum() == (deep & applies).sum() == cnt[0]["undecided"]
    assert (v[~deep, 0] == ref[~deep, 0]).all()


def test_pattern_leaf_and_exception(oracle):
    pols, excs = J.pattern_and_exception_set()
    nd = _nd(0xF6, 2)
    ps = K.PolicySet(pols, excs)
    v, _, _ = K.Engine(ordinal=0).evaluate(ps, K.Corpus(nd))
    ref = oracle.validate(pols, nd, nthreads=8, exceptions=excs)
    assert (v == 7).sum() == 0 and (v == 6).sum() == 0
    _assert_equal(v, ref, ps.rule_names)
    plain = oracle.validate(pols, nd, nthreads=8)
    assert (ref != plain).any(), "the exception's conditions hold on some rows"
    for r in range(v.shape[1]):
        assert len(set(np.unique(v[:, r]).tolist()) - {0}) >= 2, ps.rule_names[r]
