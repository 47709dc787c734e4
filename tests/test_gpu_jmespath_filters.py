"""JMESPath filter steps `[?P]` evaluated by kpe_cond_kernel: bit-exact verdict matrices against
the oracle on synthetic corpora (4096 rows: 64 full waves) with the edge documents of
tests/jmespath_filter_cases.py riding in a partial wave, the list-capacity pair, the reference's
test/cli/test/foreach scenario with its messages, and a filter inside an exception condition and
a pattern leaf variable. The host build of the same VM text is tests/test_jmespath_filters.py."""
import json

import numpy as np
import pytest

import kyverno_amd as K
from tests import jmespath_filter_cases as F

pytestmark = pytest.mark.gpu


def _nd(seed, mix):
    return K.synth_resources(seed, 4096, mix=mix).rstrip(b"\n") + b"\n" + F.edge_ndjson()


def _assert_equal(v, ref, names):
    assert v.shape == ref.shape
    bad = np.argwhere(v != ref)
    assert bad.size == 0, f"{len(bad)} mismatching cells, first {[(int(i), names[j]) for i, j in bad[:5]]} " \
                          f"gpu={[int(v[i, j]) for i, j in bad[:5]]} ref={[int(ref[i, j]) for i, j in bad[:5]]}"


@pytest.mark.parametrize("mix,seed", [(1, 0xE1), (2, 0xE2)])
def test_filters_bit_exact(oracle, mix, seed):
    pols = F.filter_policy_set()
    nd = _nd(seed, mix)
    ps = K.PolicySet(pols)
    v, _, cnt = K.Engine(ordinal=0).evaluate(ps, K.Corpus(nd))
    ref = oracle.validate(pols, nd, nthreads=8)
    assert v.shape[0] == 4096 + len(F.edge_documents())
    assert (ref == 7).sum() == 0
    assert (v == 7).sum() == 0 and (v == 6).sum() == 0
    _assert_equal(v, ref, ps.rule_names)
    for r in range(v.shape[1]):
        col = v[:, r]
        assert len(set(np.unique(col).tolist()) - {0}) >= 2, ps.rule_names[r]
        assert cnt[r]["pass"] == int((col == 1).sum()) and cnt[r]["fail"] == int((col == 2).sum())
        assert cnt[r]["error"] == int((col == 4).sum()) and cnt[r]["skip"] == int((col == 5).sum())
        assert cnt[r]["undecided"] == 0


def test_survivors_bound_the_list(oracle):
    """33 survivors of [?name != 'zz'] overflow the VM's list: exactly those cells are undecided;
    two survivors of 40 containers are decided like the oracle."""
    pols = F.overflow_policy()
    nd = b"\n".join(json.dumps(d).encode() for d in F.overflow_documents())
    v, _, cnt = K.Engine(ordinal=0).evaluate(K.PolicySet(pols), K.Corpus(nd))
    ref = oracle.validate(pols, nd)
    und = np.zeros(ref.shape, dtype=bool)
    for i, j in F.OVERFLOW_UNDECIDED:
        und[i, j] = True
    assert ((v == 7) == und).all(), v.tolist()
    assert (v[~und] == ref[~und]).all(), (v.tolist(), ref.tolist())
    assert ref[1, 1] == 2 and cnt[0]["undecided"] == 2 and cnt[1]["undecided"] == 0


def test_pattern_leaf_and_exception(oracle):
    pols, excs = F.pattern_and_exception_set()
    nd = _nd(0xE4, 2)
    ps = K.PolicySet(pols, excs)
    v, _, _ = K.Engine(ordinal=0).evaluate(ps, K.Corpus(nd))
    ref = oracle.validate(pols, nd, nthreads=8, exceptions=excs)
    assert (v == 7).sum() == 0 and (v == 6).sum() == 0
    _assert_equal(v, ref, ps.rule_names)
    plain = oracle.validate(pols, nd, nthreads=8)
    assert (ref != plain).any(), "the exception's conditions hold on some rows"
    for r in range(v.shape[1]):
        assert len(set(np.unique(v[:, r]).tolist()) - {0}) >= 2, ps.rule_names[r]


def test_cli_foreach_scenario(oracle):
    """test/cli/test/foreach on the device, all four policies: the reference's recorded results,
    the oracle's matrix, and for every cell the message rendered from kpe_fetch_cond_traces_ex /
    kpe_pattern_traces through kpe_report_results_ex (the element node of a filtered list)."""
    from tests.oracle_lib import STATUS
    from tests.test_foreach_messages import NEEDS, _gpu_messages
    from tests.test_jmespath_filters import CLI_FOREACH as case, cli_results_hold
    from tests.test_oracle_golden import cli_expectations

    pols = case["policies"]
    lines = [json.dumps(r).encode() for r in case["resources"]]
    nd = b"\n".join(lines)
    eng = K.Engine(ordinal=0)
    ps = K.PolicySet(pols)
    assert ps.num_rules == len(oracle.rule_names(pols))
    corpus = K.Corpus(nd)
    v, _, _ = eng.evaluate(ps, corpus)
    M, exp = cli_expectations(oracle, case)
    assert (v == M).all(), (v.tolist(), M.tolist())
    cli_results_hold(case, v, exp, STATUS)
    rows = list(range(len(lines)))
    om = oracle.pattern_messages(pols, nd)
    got = _gpu_messages(eng, ps, corpus, v, lines, rows)
    failing = 0
    for i in rows:
        for r in range(ps.num_rules):
            if v[i, r] in (0, 7):
                continue
            if om[i][r] == NEEDS:
                continue
            assert got[(i, r)] == om[i][r], (i, ps.rule_names[r], got[(i, r)], om[i][r])
            failing += v[i, r] in (2, 4)
    assert failing >= 4
