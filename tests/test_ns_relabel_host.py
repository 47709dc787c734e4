"""Namespace label changes on a flattened corpus, the host half (no GPU): the table edit of
kpe_corpus_set_namespace_labels (patch, replace, removal, duplicate keys, values that are no
labels, malformed input, the changed count), its getter, the host consumers of the table
(kpe_cli_summary_ns, the namespace fold) against a fresh flatten, the stand-alone sanitizer check of
the rebuilt columns (scripts/nsl_check.cpp) and the scanner's Namespace-object events."""
import copy
import ctypes
import json
import subprocess

import numpy as np
import pytest

import kyverno_amd as K
from kyverno_amd._lib import KpeError, load
from tests.conftest import build_host_tool
from tests.policies import restricted_latest, selector_policy

L0 = {"ns-a": {"env": "prod", "team": "t1"}, "ns-b": {"env": "dev"}, "ns-c": {}, "elsewhere": {"x": "y"}}


def _res(kind, name, ns=None, api="v1"):
    meta = {"name": name}
    if ns is not None:
        meta["namespace"] = ns
    d = {"apiVersion": api, "kind": kind, "metadata": meta}
    if kind == "Pod":
        d["spec"] = {"containers": [{"name": "c", "image": "x", "securityContext": {"privileged": name.endswith("1")}}]}
    return d


def _nd():
    rows = [_res("Pod", f"p{i}", ns) for i, ns in enumerate(["ns-a", "ns-b", "ns-c", "ns-d", "ns-a", "ns-b"])]
    rows += [_res("PersistentVolume", "pv"), _res("Namespace", "ns-a")]
    return "\n".join(json.dumps(r) for r in rows).encode()


def _set(c, labels, replace=False):
    """The corpus is not uploaded: the call takes no device and the table changes on the host."""
    return c.set_namespace_labels(labels, replace)


def test_symbols_exported():
    L = load()
    assert hasattr(L, "kpe_corpus_set_namespace_labels") and hasattr(L, "kpe_corpus_namespace_labels")
    assert K.NSL_REPLACE == 1


def test_getter_round_trips_in_table_order():
    c = K.Corpus(_nd(), L0)
    assert c.namespace_labels() == L0 and list(c.namespace_labels()) == list(L0)
    assert K.Corpus(_nd()).namespace_labels() == {}
    # the length convention: the size needed is returned, at most cap bytes are written
    L = load()
    n = L.kpe_corpus_namespace_labels(c.h, None, 0)
    buf = (json.dumps(L0, separators=(",", ":"))).encode()
    assert n == len(buf)
    small = ctypes.create_string_buffer(b"#" * 16, 16)
    assert L.kpe_corpus_namespace_labels(c.h, small, 8) == n and small.raw == buf[:8] + b"#" * 8
    # given back as a replacement it is the identity, on this corpus and on one without a table
    assert _set(c, c.namespace_labels(), replace=True) == 0
    d = K.Corpus(_nd())
    assert _set(d, c.namespace_labels(), replace=True) == len(L0) and d.namespace_labels() == L0
    assert list(d.namespace_labels()) == list(L0)
    odd = {'q"uote\\': {"ké\t": "v\n"}}
    assert _set(d, odd) == 1 and d.namespace_labels()['q"uote\\'] == odd['q"uote\\']


def test_patch_sets_removes_and_keeps():
    c = K.Corpus(_nd(), L0)
    G, rows, nbytes = c.namespaces, c.row_namespaces().copy(), c.nbytes
    n = _set(c, {"ns-a": {"env": "staging", "new-key": "new-value"}, "ns-b": None, "ns-d": {"env": "prod"},
                 "ns-c": {}, "nowhere": None})
    assert n == 3  # ns-a changed, ns-b removed, ns-d added; ns-c equal, nowhere was not there
    want = {"ns-a": {"env": "staging", "new-key": "new-value"}, "ns-c": {}, "elsewhere": {"x": "y"}, "ns-d": {"env": "prod"}}
    assert c.namespace_labels() == want and list(c.namespace_labels()) == list(want)
    # a namespace only the table names is no group; the groups and the rows' groups do not move
    assert c.namespaces == G and np.array_equal(c.row_namespaces(), rows)
    assert c.nbytes == nbytes  # four entries and five labels, before and after
    assert _set(c, {"big": {"a": "1", "b": "2"}}) == 1 and _set(c, {"big": None}) == 1 and _set(c, {"big": {"a": "1", "b": "2"}}) == 1
    assert c.nbytes == nbytes + 4 * (1 + 2 + 2) == load().kpe_corpus_bytes(c.h)  # one row offset, two key and value ids
    want["big"] = {"a": "1", "b": "2"}
    assert _set(c, None) == 0 and _set(c, b"") == 0 and _set(c, {}) == 0 and c.namespace_labels() == want


def test_replace_is_what_flatten_builds():
    c = K.Corpus(_nd(), L0)
    new = {"ns-d": {"a": "b"}, "ns-a": {"team": "t1", "env": "prod"}}
    assert _set(c, new, replace=True) == 4  # ns-b, ns-c, elsewhere go, ns-d comes; ns-a: an equal set
    assert c.namespace_labels() == K.Corpus(_nd(), new).namespace_labels()
    assert list(c.namespace_labels()) == ["ns-d", "ns-a"]
    for empty in (None, b"", {}, b"null"):
        d = K.Corpus(_nd(), L0)
        assert _set(d, empty, replace=True) == len(L0) and d.namespace_labels() == {}
    assert _set(K.Corpus(_nd()), {}, replace=True) == 0


def test_values_are_read_as_flatten_reads_them():
    raw = (b'{"ns-a": {"env": "qa", "n": 7, "o": {"x": "y"}, "l": ["a"], "t": true, "z": null, "s": "str"},'
           b' "ns-b": 5, "ns-c": "text", "ns-d": ["x"], "ns-e": true}')
    c = K.Corpus(_nd(), L0)
    assert _set(c, raw) == 4  # ns-c had no labels and has none
    assert c.namespace_labels() == K.Corpus(_nd(), raw).namespace_labels() | {"elsewhere": {"x": "y"}}
    got = c.namespace_labels()
    assert got["ns-a"] == {"env": "qa", "s": "str"} and got["ns-b"] == {} and got["ns-d"] == {} and got["ns-e"] == {}
    # replace: null is a value that is no object (an entry without labels), as in a flatten
    d = K.Corpus(_nd(), L0)
    _set(d, b'{"ns-a": null, "ns-x": {"k": "v"}}', replace=True)
    assert d.namespace_labels() == {"ns-a": {}, "ns-x": {"k": "v"}} == K.Corpus(_nd(), b'{"ns-a": null, "ns-x": {"k": "v"}}').namespace_labels()


def test_duplicate_key_counts_by_its_last_occurrence():
    c = K.Corpus(_nd(), L0)
    assert _set(c, b'{"ns-a": {"env": "one"}, "ns-b": null, "ns-a": {"env": "two"}, "ns-b": {"env": "back"}}') == 2
    got = c.namespace_labels()
    assert got["ns-a"] == {"env": "two"} and got["ns-b"] == {"env": "back"}
    c = K.Corpus(_nd(), L0)
    assert _set(c, b'{"ns-a": {"env": "one"}, "ns-a": null}') == 1 and "ns-a" not in c.namespace_labels()
    c = K.Corpus(_nd(), L0)
    assert _set(c, b'{"ns-q": {"a": "1"}, "ns-q": {"a": "2"}}', replace=True) == 5
    assert c.namespace_labels() == {"ns-q": {"a": "2"}}


def test_changed_counts_sets_not_order():
    c = K.Corpus(_nd(), L0)
    assert _set(c, {"ns-a": {"team": "t1", "env": "prod"}}) == 0
    assert _set(c, b'{"ns-a": {"team": "t1", "env": "prod", "team": "t1"}}') == 0  # the same set of pairs
    assert list(c.namespace_labels()["ns-a"]) == ["env", "team"]  # untouched
    assert _set(c, {"ns-a": {"team": "t1", "env": "prod", "more": "x"}}) == 1
    assert _set(c, {"ns-a": {"team": "t1"}}) == 1
    assert _set(c, dict(reversed(list(c.namespace_labels().items()))), replace=True) == 0


@pytest.mark.parametrize("bad", [b'{"ns-a": {"env": "x"}', b'[{"ns-a": {}}]', b'"text"', b"7", b'{"ns-a": {"env": }}',
                                 b'{"ns-a" {"env": "x"}}', b"{,}"])
@pytest.mark.parametrize("replace", [False, True])
def test_malformed_is_invalid_and_changes_nothing(bad, replace):
    c = K.Corpus(_nd(), L0)
    digest = c.digest()
    with pytest.raises(KpeError) as e:
        _set(c, bad, replace)
    assert e.value.status == 1  # KPE_E_INVALID
    assert c.namespace_labels() == L0 and c.digest() == digest
    n = ctypes.c_uint64(77)
    assert load().kpe_corpus_set_namespace_labels(None, c.h, b"{}", 2, 6, ctypes.byref(n)) == 1  # unknown flag
    assert load().kpe_corpus_set_namespace_labels(None, None, b"{}", 2, 0, None) == 1


def test_nsl_check_tool():
    """The rebuilt table and every row's table row equal a fresh flatten's by namespace name and
    label strings, over 0, 1 and 3000 rows, under ASan / UBSan (scripts/nsl_check.cpp)."""
    tool = build_host_tool("nsl_check")
    r = subprocess.run([tool], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "nsl_check ok" in r.stdout, r.stdout + r.stderr


# ---- the host consumers of the table ----
def _override_policies():
    """validationFailureActionOverrides by namespaceSelector (the action of kpe_cli_summary_ns) and a
    rule whose match reads the namespace labels."""
    p = copy.deepcopy(restricted_latest())
    p["spec"]["validationFailureActionOverrides"] = [{"action": "Enforce", "namespaceSelector": {"matchLabels": {"env": "prod"}}}]
    q = selector_policy("ns-prod", kinds=("Pod",), ns_selector={"matchLabels": {"env": "prod"}})
    q["spec"]["validationFailureActionOverrides"] = [{"action": "Enforce", "namespaceSelector": {"matchExpressions": [
        {"key": "team", "operator": "Exists"}]}}]
    return [p, q]


@pytest.fixture(scope="module")
def consumer_case(oracle):
    nd = K.synth_resources(0xC3, 400, mix=K.SYNTH_C3)
    docs = [json.loads(x) for x in nd.split(b"\n") if x.strip()]
    names = sorted({(d.get("metadata") or {}).get("namespace", "") for d in docs} - {""})
    la = {ns: ({"env": "prod", "team": "a"} if i % 2 else {"env": "dev"}) for i, ns in enumerate(names)}
    lb = {ns: ({"env": "prod"} if i % 3 == 0 else {"env": "dev", "team": "b"}) for i, ns in enumerate(names) if i % 5}
    pols = _override_policies()
    return nd, la, lb, pols, oracle.validate(pols, nd, ns_labels=la, nthreads=4), oracle.validate(pols, nd, ns_labels=lb, nthreads=4)


@pytest.mark.parametrize("replace", [False, True])
def test_cli_summary_ns_and_fold_follow_the_relabel(consumer_case, replace):
    nd, la, lb, pols, va, vb = consumer_case
    assert (va != vb).any() and (vb == 2).any()
    ps = K.PolicySet(pols)
    c = K.Corpus(nd, la)
    old = K.cli_summary_ns(ps, c, K.namespace_counts(ps, c, va), True)
    patch = lb if replace else {**lb, **{ns: None for ns in la if ns not in lb}}
    assert _set(c, patch, replace) == len(la)
    fresh = K.Corpus(nd, lb)
    assert c.namespace_labels() == fresh.namespace_labels()
    t_c, t_f = K.namespace_counts(ps, c, vb), K.namespace_counts(ps, fresh, vb)
    assert c.namespaces == fresh.namespaces and np.array_equal(t_c, t_f)
    for aw in (False, True):
        assert K.cli_summary_ns(ps, c, t_c, aw) == K.cli_summary_ns(ps, fresh, t_f, aw)
    new = K.cli_summary_ns(ps, c, t_c, True)
    assert new != old  # or the labels decided nothing
    # the action alone follows the labels too: the old matrix under the new table
    assert K.cli_summary_ns(ps, c, K.namespace_counts(ps, c, va), True) == \
        K.cli_summary_ns(ps, fresh, K.namespace_counts(ps, fresh, va), True) != old


def test_absent_entry_and_empty_entry_are_the_same_to_consumers(consumer_case):
    nd, la, _, pols, va, _ = consumer_case
    ps = K.PolicySet(pols)
    a, b = K.Corpus(nd, la), K.Corpus(nd, la)
    some = list(la)[:7]
    _set(a, {ns: None for ns in some})
    _set(b, {ns: {} for ns in some})
    assert a.namespace_labels() != b.namespace_labels()
    for aw in (False, True):
        assert K.cli_summary_ns(ps, a, K.namespace_counts(ps, a, va), aw) == K.cli_summary_ns(ps, b, K.namespace_counts(ps, b, va), aw)


# ---- the scanner's Namespace-object events (no device) ----
def test_namespace_label_events():
    ev = K.namespace_label_events
    ns = lambda name, labels=None, api="v1": {"apiVersion": api, "kind": "Namespace",  # noqa: E731
                                              "metadata": {"name": name, **({"labels": labels} if labels is not None else {})}}
    ups = [json.dumps(ns("a", {"env": "prod", "n": 7, "o": {"x": 1}})).encode(), json.dumps(_res("Pod", "p", "a")).encode(),
           json.dumps(ns("b")).encode(), json.dumps(ns("c", {"k": "v"}, api="example.io/v1")).encode(), b"not json", b"[1]",
           json.dumps(ns("a", {"env": "dev"})).encode(), json.dumps({"apiVersion": "v1", "kind": "Namespace"}).encode(),
           json.dumps(ns("d", ["x"])).encode()]
    assert ev(ups) == {"a": {"env": "dev"}, "b": {}, "d": {}}
    assert ev([ns("a", {"env": "prod", "n": 7})]) == {"a": {"env": "prod"}}  # parsed resources too
    gone = [json.dumps(ns("a", {"env": "prod"})).encode(), ("v1", "Namespace", None, "z"), ("v1", "Pod", "a", "p"),
            ("uid", "1234"), ("apps/v1", "Namespace", None, "y"), ns("w"), 17]
    assert ev(ups, gone) == {"a": None, "b": {}, "d": {}, "z": None, "w": None}
    assert ev() == {}
    with pytest.raises(ValueError):
        K.ResidentScanner(None, b"", ns_objects=True)  # only with keyed=True; refused before any device call
