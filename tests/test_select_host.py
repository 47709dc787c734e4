"""Sparse result fetch, host half (no GPU): the three entry points are exported, the host
summary fold (kpe_row_summaries_host) agrees with kpe_report_results, the project's
restatement of EngineResponseToReportResults that test_report.py pins to the oracle
(CalculateSummary, pkg/utils/report/results.go:39-55, counts those results' `result`
values), and the argument checks that come before any device call."""
import collections
import copy
import ctypes

import numpy as np
import pytest

import kyverno_amd as K
from kyverno_amd._lib import load
from tests.policies import parity_policy_set, pss_policy

CODES = (0, 1, 2, 3, 4, 5, 7)  # the kpe_verdict alphabet
KPE_E_INVALID, KPE_E_LIMIT = 1, 4


def summary_policy_set():
    """The first policies of parity_policy_set, one of them unscored, plus an unscored policy of
    its own (policies.kyverno.io/scored: "false": its fails are warns, results.go:131-133)."""
    pols = copy.deepcopy(parity_policy_set()[:5])
    pols[1]["metadata"]["annotations"] = {"policies.kyverno.io/scored": "false"}
    p = pss_policy("unscored", "restricted")
    p["metadata"]["annotations"] = {"policies.kyverno.io/scored": "false"}
    return pols + [p]


def all_codes_matrix(R):
    """Every code of the alphabet in every column, shifted per column so that rows mix codes."""
    n = len(CODES) * 3
    v = np.zeros((n, R), dtype=np.uint8)
    for i in range(n):
        for r in range(R):
            v[i, r] = CODES[(i + r) % len(CODES)] if i < 2 * len(CODES) else CODES[(i * 5 + r * 3) % len(CODES)]
    for r in range(R):
        assert set(v[:, r].tolist()) == set(CODES)
    return v


def test_symbols_exported():
    L = load()
    for name in ("kpe_select_cells", "kpe_fetch_row_summaries", "kpe_row_summaries_host"):
        assert hasattr(L, name), name
    assert callable(K.row_summaries)
    assert K.SEL_RESPONSES == 0xFE and K.SEL(2) == 4
    assert K.SUMMARY_FIELDS == ("pass", "fail", "warn", "error", "skip", "undecided")


def test_host_fold_matches_report_results():
    pols = summary_policy_set()
    ps = K.PolicySet(pols)
    R = ps.num_rules
    v = all_codes_matrix(R)
    got = K.row_summaries(ps, v)
    assert got.shape == (v.shape[0], 6) and got.dtype == np.uint16
    unscored = np.array([n.split("/", 1)[0] in ("pol-unscored", pols[1]["metadata"]["name"]) for n in ps.rule_names])
    assert unscored.any() and not unscored.all()
    saw_unscored_fail = False
    for i in range(v.shape[0]):
        results = K.report_results(ps, v[i])
        ref = collections.Counter(r["result"] for r in results)
        assert set(ref) <= {"pass", "fail", "warn", "error", "skip"}
        row = dict(zip(K.SUMMARY_FIELDS, (int(x) for x in got[i])))
        for k in ("pass", "fail", "warn", "error", "skip"):
            assert row[k] == ref.get(k, 0), (i, k, row, ref)
        assert row["undecided"] == int((v[i] == 7).sum())
        # NA lands nowhere: the counters add up to the cells that are not NA
        assert sum(row.values()) == int((v[i] != 0).sum())
        # an unscored FAIL is a warn, a scored one a fail
        uf = int(((v[i] == 2) & unscored).sum())
        saw_unscored_fail |= uf > 0
        assert row["warn"] == uf + int((v[i] == 3).sum())
        assert row["fail"] == int(((v[i] == 2) & ~unscored).sum())
    assert saw_unscored_fail
    # a single row given as a vector
    assert np.array_equal(K.row_summaries(ps, v[3]), got[3:4])
    assert K.row_summaries(ps, np.zeros((0, R), dtype=np.uint8)).shape == (0, 6)


def test_select_argument_errors_without_device():
    L = load()
    ps = K.PolicySet(summary_policy_set())
    corpus = K.Corpus([{"apiVersion": "v1", "kind": "Pod", "metadata": {"name": "a"}}])
    sel = (ctypes.c_uint8 * ps.num_rules)(*([0xFE] * ps.num_rules))
    cells = (ctypes.c_uint64 * 4)()
    # NULL device
    assert L.kpe_select_cells(None, ps.h, corpus.h, sel, cells, None, 4) == -KPE_E_INVALID
    # sel == NULL and cap > 0 without cells: checked before any device call, so any non-NULL
    # device handle will do (it is never dereferenced)
    fake_dev = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    assert L.kpe_select_cells(fake_dev, ps.h, corpus.h, None, cells, None, 4) == -KPE_E_INVALID
    assert L.kpe_select_cells(fake_dev, ps.h, corpus.h, sel, None, None, 4) == -KPE_E_INVALID
    assert L.kpe_last_error()


def test_row_summaries_argument_errors_without_device():
    L = load()
    ps = K.PolicySet(summary_policy_set())
    out = np.zeros((2, 6), dtype=np.uint16)
    v = np.zeros((2, ps.num_rules), dtype=np.uint8)
    assert L.kpe_row_summaries_host(None, v.ctypes.data, 2, out.ctypes.data) == KPE_E_INVALID
    assert L.kpe_row_summaries_host(ps.h, None, 2, out.ctypes.data) == KPE_E_INVALID
    assert L.kpe_row_summaries_host(ps.h, v.ctypes.data, 2, None) == KPE_E_INVALID
    assert L.kpe_row_summaries_host(ps.h, None, 0, None) == 0
    corpus = K.Corpus([{"apiVersion": "v1", "kind": "Pod", "metadata": {"name": "a"}}])
    assert L.kpe_fetch_row_summaries(None, ps.h, corpus.h, 0, 1, out.ctypes.data) == KPE_E_INVALID
    with pytest.raises(ValueError):
        K.row_summaries(ps, np.zeros((2, ps.num_rules + 1), dtype=np.uint8))
