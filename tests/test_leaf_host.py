"""The pattern-leaf table (tests/leaf_cases.py) through the host build of the pattern VM
(scripts/patvm_check: patvm.inl + strmatch.inl under AddressSanitizer / UBSan with bounds flags,
run stand-alone). Every cell must equal the oracle's, the reference's own vectors must give their
`want`, the tool must end with status 0 and no cell may be undecided. The tool evaluates each
leaf four ways (lane-private stack, LDS stack, deferred deep walk, leaf table) and fails when
they differ. CPU only."""
import json
import subprocess

import numpy as np
import pytest

from tests import leaf_cases as L


@pytest.fixture(scope="module")
def harness():
    from tests.conftest import build_host_tool

    return build_host_tool("patvm_check")


def run_tool(harness, tmp_path, pols, nd):
    pj, rj, vb = tmp_path / "p.json", tmp_path / "r.ndjson", tmp_path / "v.bin"
    pj.write_text(json.dumps(pols, ensure_ascii=False))
    rj.write_bytes(nd)
    r = subprocess.run([harness, str(pj), str(rj), str(vb)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    n, R, err, nscal = r.stdout.split()
    assert err == "err=0x0"
    return np.fromfile(vb, dtype=np.uint8).reshape(int(n), int(R)), int(nscal.split("=")[1])


def test_golden_vectors_kept():
    """51 of the 64 Validate vectors have scalars on both sides; with the string-leaf vectors of
    pattern_test.go and the 52 ext/wildcard pairs, every vector but the listed ones is in the table."""
    _, _, want, ngold, nvalidate = L.table()
    total = sum(c["fn"] in ("pattern", "patterns", "string", "compare") for c in L.PLEAF) + nvalidate + len(L.WILD["match"])
    assert nvalidate == 51 and len(L.WILD["match"]) == 52
    assert ngold >= total - len(L.DROPPED) and len(L.DROPPED) <= 8
    assert len(want) >= 140  # distinct cells (some vectors repeat a pair)


def test_leaf_table_host(harness, oracle, tmp_path):
    pats, vals, want, _, _ = L.table()
    pols, nd = L.policies(pats), L.ndjson(vals)
    v, _ = run_tool(harness, tmp_path, pols, nd)
    ref = oracle.validate(pols, nd, nthreads=8)
    assert v.shape == ref.shape == (len(vals), len(pats))
    assert set(np.unique(ref)) <= {1, 2}  # every leaf applies to every document
    assert not (v == 7).any()
    bad = np.argwhere(v != ref)
    assert bad.size == 0, f"{len(bad)} cells differ, first " \
                          f"{[(vals[i], pats[j], int(v[i, j]), int(ref[i, j])) for i, j in bad[:8]]}"
    wrong = [(name, pats[j], vals[i], w, int(v[i, j])) for (j, i), (name, w) in want.items() if v[i, j] != (1 if w else 2)]
    assert not wrong, wrong[:8]
    # both verdicts are common: the table is not decided by one answer
    assert 0.1 < (ref == 1).mean() < 0.9


@pytest.mark.parametrize("nscal", L.SCALAR_COUNTS)
def test_scalar_counts_as_derived(harness, tmp_path, nscal):
    """The truncated document lists of the device test intern exactly the scalars the test believes
    (leaf_cases.scalar_count); the tool prints the flattener's own count."""
    vals = L.simple_head(nscal - 7) + ["7777"]  # the last scalar is a number the `>` forms pass
    assert L.scalar_count(vals) == nscal
    _, got = run_tool(harness, tmp_path, L.policies(L.patterns()[:40]), L.ndjson(vals))
    assert got == nscal


def test_aligned_tails_host(harness, oracle, tmp_path):
    """The last scalar text at each of the 8 byte alignments, ending the text buffer (the VM's 8-byte
    loads read into the slack behind it): longest and shortest string last."""
    pats = [p for p in L.patterns() if any(c in p for c in "*?") or not p.isascii()]
    pols = L.policies(pats)
    for vals in L.aligned_tails():
        nd = L.ndjson(vals)
        v, _ = run_tool(harness, tmp_path, pols, nd)
        assert np.array_equal(v, oracle.validate(pols, nd))


def test_zero_valued_pattern_is_a_validate_rule(harness, oracle, tmp_path):
    """HasValidate (rule_types.go:164-166) is !DeepEqual(Validation, Validation{}) and the raw pattern is a
    pointer: a pattern whose every leaf is a zero value, or the empty map, still makes a validate rule
    that answers. The leaf verdicts are the reference's own (pattern_test.go TestValidate[1], [3]:
    pattern false against true fails, against false passes); the empty map pattern passes anything."""
    pols = L.policies(["false", '""', "0", "null"]) + [json.loads(L.policy(9, "0"))]
    pols[-1]["spec"]["rules"][0]["validate"]["pattern"] = {}
    nd = L.ndjson(["true", "false"])
    ref = oracle.validate(pols, nd)
    assert ref[:, 0].tolist() == [2, 1] and ref[:, 4].tolist() == [1, 1] and (ref != 0).all()
    v, _ = run_tool(harness, tmp_path, pols, nd)
    assert np.array_equal(v, ref)
