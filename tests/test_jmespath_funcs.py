"""go-jmespath builtins in device queries: contains, starts_with, ends_with, not_null, values()
and keys() in function form (oracle/conditions.hpp Interp::call is the specification).

CPU: what kpe_program_compile accepts and still refuses, and the condition VM compiled for the
host under ASan/UBSan (scripts/condvm_check.cpp, the text kpe_cond_kernel runs) against the oracle
on a synthetic corpus plus hand-written edge documents. The device run of the same set is
tests/test_gpu_jmespath_funcs.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import kyverno_amd as K
from tests import jmespath_func_cases as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _deny_pol(cond):
    return J.policy("p", [J.rule("r", J.deny(cond), kinds=("Pod",))])


@pytest.mark.parametrize("name,cond", J.DENY_CONDITIONS, ids=[n for n, _ in J.DENY_CONDITIONS])
def test_condition_compiles(oracle, name, cond):
    pols = [_deny_pol(cond)]
    assert K.PolicySet(pols).rule_names == oracle.rule_names(pols)


def test_sets_compile(oracle):
    for pols in (J.func_policy_set(), J.needle_list_policy()):
        assert K.PolicySet(pols).rule_names == oracle.rule_names(pols)
    pols, excs = J.pattern_and_exception_set()  # a pattern leaf, a pattern template, an exception condition
    assert K.PolicySet(pols, excs).rule_names == oracle.rule_names(pols)
    # a pattern key variable
    key = [J.policy("k", [J.rule("r", {"pattern": {"metadata": {"labels": {
        J.q(f"not_null({J.LABELS}.which, 'app')"): "?*"}}}}, kinds=("Pod",))])]
    assert K.PolicySet(key).rule_names == oracle.rule_names(key)


@pytest.mark.parametrize("expr", [
    f"to_string({J.NAME})",                      # json.Marshal text: not on the device
    f"contains({J.NAME})",                       # arity
    f"contains({J.NAME}, 'a', 'b')",
    f"starts_with({J.NAME})",
    "not_null()",
    f"contains(length({J.NAME}), `1`)",          # a call inside an argument other than keys / values
    f"contains(keys(length({J.NAME})), `1`)",
    f"contains(to_string({J.NAME}), '1')",
    f"not_null(contains({J.NAME}, 'a'), `true`)",
    f"{J.NAME} | starts_with(@, 'x')",           # a pipe into a call
    f"contains({J.NAME}, 'a') | length(@)",
    f"contains({J.NAME}, 'a').x",                # steps after a call
    f"contains({J.NAME}, 'a')[0]",
    f"keys({J.OBJ}.spec.containers[*])",         # keys() / values() of a projection
    f"values({J.LABELS}).x",
    f"contains({J.NAME}, 'a' 'b')",              # no comma
    f"contains({J.NAME}, )",
    f"contains({J.OBJ}.spec.containers[?name == 'a'], 'x')",  # filters, comparators, !, && stay refused
    f"contains({J.NAME}, 'a') && `true`",
    f"!contains({J.NAME}, 'a')",
    f"contains({J.NAME}, 'a') == `true`",
    f"to_upper({J.NAME})",
    f"contains(request.userInfo.username, 'a')",
])
def test_still_refused(expr):
    with pytest.raises(K.KpeError) as e:
        K.PolicySet([_deny_pol(J.c(J.q(expr), "Equals", True))])
    assert e.value.status == 2


# ---- the host build of the condition VM against the oracle ------------------------------------

@pytest.fixture(scope="module")
def condvm_bin():
    from tests.conftest import build_host_tool

    return build_host_tool("condvm_check")


def _corpus(seed):
    lines = [l for l in K.synth_resources(seed, 2500, mix=2).split(b"\n") if l and json.loads(l)["kind"] in J.KINDS]
    lines += J.edge_ndjson().split(b"\n")
    return lines


def _run_host(condvm_bin, tmp_path, pols, lines):
    """condvm_check over cells seeded the way the scan kernel would (6: a matched condition rule)."""
    rules = pols[0]["spec"]["rules"]
    kinds = [json.loads(l)["kind"] for l in lines]
    seedm = np.zeros((len(lines), len(rules)), dtype=np.uint8)
    for j, r in enumerate(rules):
        rk = set(r["match"]["any"][0]["resources"]["kinds"])
        seedm[:, j] = [6 if k in rk else 0 for k in kinds]
    (tmp_path / "p.json").write_text(json.dumps(pols))
    (tmp_path / "r.ndjson").write_bytes(b"\n".join(lines))
    (tmp_path / "seed.bin").write_bytes(seedm.tobytes())
    subprocess.check_call([condvm_bin, str(tmp_path / "p.json"), str(tmp_path / "r.ndjson"),
                           str(tmp_path / "seed.bin"), str(tmp_path / "out.bin")])
    return np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.uint8).reshape(seedm.shape)


def test_host_vm_matches_oracle(condvm_bin, oracle, tmp_path):
    pols = J.func_policy_set()
    names = [r["name"] for r in pols[0]["spec"]["rules"]]
    lines = _corpus(0xF1)
    ref = oracle.validate(pols, b"\n".join(lines), nthreads=8)
    assert ref.shape == (len(lines), len(names))
    assert (ref == 7).sum() == 0, "no row of this corpus has a context error"
    for j, n in enumerate(names):  # not vacuous: every rule decides both ways (or errors) somewhere
        assert len(set(np.unique(ref[:, j]).tolist()) - {0}) >= 2, (n, np.unique(ref[:, j]).tolist())
    out = _run_host(condvm_bin, tmp_path, pols, lines)
    assert (out == 7).sum() == 0
    for j, n in enumerate(names):
        bad = np.nonzero(out[:, j] != ref[:, j])[0]
        assert bad.size == 0, (n, bad[:5].tolist(), out[bad[:5], j].tolist(), ref[bad[:5], j].tolist(),
                               [lines[i][:200] for i in bad[:2]])


def test_host_vm_list_needle_is_undecided(condvm_bin, oracle, tmp_path):
    pols = J.needle_list_policy()
    lines = _corpus(0xF2)
    docs = [json.loads(l) for l in lines]
    deep = np.array(J.needle_list_rows(docs))
    assert 0 < deep.sum() < len(lines)
    ref = oracle.validate(pols, b"\n".join(lines), nthreads=8)
    out = _run_host(condvm_bin, tmp_path, pols, lines)
    assert (out[deep, 0] == 7).all()
    assert (out == 7).sum() == deep.sum()
    assert (out[~deep, 0] == ref[~deep, 0]).all()
    assert {1, 2} <= set(np.unique(ref[:, 0]).tolist())
