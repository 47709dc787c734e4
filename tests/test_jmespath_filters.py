"""JMESPath filter steps `[?P]` in device queries (oracle/conditions.hpp Parser::filter and
Interp::eval N_FILTER / N_CMP / N_AND / N_OR / N_NOT are the specification).

CPU: what kpe_program_compile accepts and still refuses, and the condition VM compiled for the
host under ASan/UBSan (scripts/condvm_check.cpp, the text kpe_cond_kernel runs) against the oracle
on a synthetic corpus plus hand-written edge documents, on the list-capacity pair and on the
reference's own test/cli/test/foreach scenario. The device run of the same sets is
tests/test_gpu_jmespath_filters.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import kyverno_amd as K
from tests import jmespath_filter_cases as F
from tests.jmespath_func_cases import c, deny, policy, q, rule

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CLI_FOREACH = [x for x in json.load(open(os.path.join(GOLD, "cli_cases.json"))) if x["name"] == "test/cli/test/foreach"][0]


def _deny_pol(cond):
    return policy("p", [rule("r", deny(cond), kinds=("Pod",))])


@pytest.mark.parametrize("name,cond", F.DENY_CONDITIONS, ids=[n for n, _ in F.DENY_CONDITIONS])
def test_condition_compiles(oracle, name, cond):
    pols = [_deny_pol(cond)]
    assert K.PolicySet(pols).rule_names == oracle.rule_names(pols)


def test_sets_compile(oracle):
    for pols in (F.filter_policy_set(), F.overflow_policy()):
        assert K.PolicySet(pols).rule_names == oracle.rule_names(pols)
    pols, excs = F.pattern_and_exception_set()  # pattern leaf variables, an exception condition
    assert K.PolicySet(pols, excs).rule_names == oracle.rule_names(pols)


@pytest.mark.parametrize("expr", F.REFUSED)
def test_still_refused(expr):
    with pytest.raises(K.KpeError) as e:
        K.PolicySet([_deny_pol(c(q(expr), "Equals", True))])
    assert e.value.status == 2


def test_filter_list_value_refused_but_foreach_list_accepted(oracle):
    """The filter's own element list: refused as a {{ }} value, accepted as a foreach list."""
    expr = F.C + "[?name == 'a']"
    with pytest.raises(K.KpeError) as e:
        K.PolicySet([_deny_pol(c(q(expr), "Equals", []))])
    assert e.value.status == 2
    for lst in (expr, expr + " || `[]`"):
        pols = [policy("p", [rule("r", {"foreach": [{"list": lst, "deny": {"conditions": {"all": [
            c(q("element.name"), "Equals", "a")]}}}]}, kinds=("Pod",))])]
        assert K.PolicySet(pols).rule_names == oracle.rule_names(pols)


# ---- the host build of the condition VM against the oracle ------------------------------------

@pytest.fixture(scope="module")
def condvm_bin():
    from tests.conftest import build_host_tool

    return build_host_tool("condvm_check")


def _run_host(condvm_bin, tmp_path, pols, lines, seedm):
    """condvm_check over cells seeded the way the scan kernel would (6: a matched condition rule)."""
    (tmp_path / "p.json").write_text(json.dumps(pols))
    (tmp_path / "r.ndjson").write_bytes(b"\n".join(lines))
    (tmp_path / "seed.bin").write_bytes(seedm.astype(np.uint8).tobytes())
    subprocess.check_call([condvm_bin, str(tmp_path / "p.json"), str(tmp_path / "r.ndjson"),
                           str(tmp_path / "seed.bin"), str(tmp_path / "out.bin")])
    return np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.uint8).reshape(seedm.shape)


def _seed_by_kind(pols, lines):
    rules = [r for p in pols for r in p["spec"]["rules"]]
    kinds = [json.loads(l)["kind"] for l in lines]
    seedm = np.zeros((len(lines), len(rules)), dtype=np.uint8)
    for j, r in enumerate(rules):
        rk = set(r["match"]["any"][0]["resources"]["kinds"])
        seedm[:, j] = [6 if k in rk else 0 for k in kinds]
    return seedm


def test_host_vm_matches_oracle(condvm_bin, oracle, tmp_path):
    pols = F.filter_policy_set()
    names = [r["name"] for r in pols[0]["spec"]["rules"]]
    lines = [l for l in K.synth_resources(0xE3, 2500, mix=2).split(b"\n") if l and json.loads(l)["kind"] in F.KINDS]
    lines += F.edge_ndjson().split(b"\n")
    ref = oracle.validate(pols, b"\n".join(lines), nthreads=8)
    assert ref.shape == (len(lines), len(names))
    assert (ref == 7).sum() == 0, "no row of this corpus has a context error"
    for j, n in enumerate(names):  # not vacuous: every rule decides both ways (or errors) somewhere
        assert len(set(np.unique(ref[:, j]).tolist()) - {0}) >= 2, (n, np.unique(ref[:, j]).tolist())
    out = _run_host(condvm_bin, tmp_path, pols, lines, _seed_by_kind(pols, lines))
    assert (out == 7).sum() == 0
    for j, n in enumerate(names):
        bad = np.nonzero(out[:, j] != ref[:, j])[0]
        assert bad.size == 0, (n, bad[:5].tolist(), out[bad[:5], j].tolist(), ref[bad[:5], j].tolist(),
                               [lines[i][:300] for i in bad[:2]])


def test_host_vm_survivors_bound_the_list(condvm_bin, oracle, tmp_path):
    """CV_LIST_CAP (32) bounds the elements that survive P, not the source list."""
    pols = F.overflow_policy()
    lines = [json.dumps(d).encode() for d in F.overflow_documents()]
    ref = oracle.validate(pols, b"\n".join(lines))
    assert (ref != 0).all() and (ref != 7).all()
    out = _run_host(condvm_bin, tmp_path, pols, lines, _seed_by_kind(pols, lines))
    und = np.zeros(ref.shape, dtype=bool)
    for i, j in F.OVERFLOW_UNDECIDED:
        und[i, j] = True
    assert ((out == 7) == und).all(), out.tolist()
    assert (out[~und] == ref[~und]).all(), (out.tolist(), ref.tolist())
    assert ref[1, 1] == 2 and ref[2, 1] == 2  # two survivors of 40, and of 3


def test_cli_foreach_scenario_on_host_vm(condvm_bin, oracle, tmp_path):
    """test/cli/test/foreach: all four policies compile, and through the host VM every result the
    reference's `kyverno test` recorded holds (mapped as tests/test_oracle_golden.py does)."""
    from tests.oracle_lib import STATUS
    from tests.test_oracle_golden import cli_expectations

    case = CLI_FOREACH
    pols = case["policies"]
    assert len(pols) == 4
    assert K.PolicySet(pols).rule_names == oracle.rule_names(pols)
    M, exp = cli_expectations(oracle, case)
    assert (M != 7).all()
    lines = [json.dumps(r).encode() for r in case["resources"]]
    out = _run_host(condvm_bin, tmp_path, pols, lines, np.where(M != 0, 6, 0))
    assert (out == M).all(), (out.tolist(), M.tolist())
    assert len(exp) == 10
    cli_results_hold(case, out, exp, STATUS)


def cli_results_hold(case, v, exp, STATUS):
    """The recorded `kyverno test` results against the verdict matrix v, as test_cli_golden maps
    them: a response must equal the expectation, and no response is accepted only for an expected
    `skip` / `fail` (output.go counts those as successes without a response)."""
    for i, cols, want, unscored, pol, rl in exp:
        got = next((g for g in (STATUS[int(v[i, k])] for k in cols) if g != "na"), "na")
        assert got != "unsupported"
        if got == "fail" and unscored:
            got = "warn"
        if got == "na":
            assert want in ("skip", "fail"), (case["resources"][i]["metadata"]["name"], pol, want)
            continue
        assert got == want, (case["resources"][i]["metadata"]["name"], pol, got, want)
