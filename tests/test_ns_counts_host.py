"""Per-namespace rule counts, host half (no GPU): the namespace groups of a corpus against a
Python parse of its NDJSON, the host fold (kpe_namespace_counts_host) against numpy, the
`kyverno apply` totals with validationFailureActionOverrides (kpe_cli_summary_ns) against a
restatement, written here, of GetValidationFailureAction (pkg/engine/api/engineresponse.go:196-225),
CheckSelector (pkg/utils/match/labels.go:10-24) and ResultCounts.addEngineResponse
(cmd/cli/kubectl-kyverno/processor/result.go:34-68) applied to the oracle's verdict matrix, and
the shard merge (merge_namespace_counts).

The issue behind this file also asks for a corpus line that is not a JSON object: the flattener
refuses such a line (KPE_E_INVALID), so no such row exists; test_groups_match_a_python_parse pins
the refusal instead, and covers rows without a namespace string with resources that have no
metadata.namespace or no metadata at all."""
import copy
import ctypes
import json
import re

import numpy as np
import pytest

import kyverno_amd as K
from kyverno_amd._lib import CliTotals, load
from kyverno_amd.shard import merge_namespace_counts
from tests.policies import parity_policy_set

CODES = (0, 1, 2, 3, 4, 5, 7)  # the kpe_verdict alphabet
FIELD_CODE = (1, 2, 3, 4, 5, 7)  # NS_COUNT_FIELDS -> verdict code
KPE_E_INVALID = 1
SENTINEL = 0xA5A5A5A5


def _pod(name, ns=None):
    meta = {"name": name}
    if ns is not None:
        meta["namespace"] = ns
    return {"apiVersion": "v1", "kind": "Pod", "metadata": meta,
            "spec": {"containers": [{"name": "c", "image": "nginx"}]}}


def hand_corpus():
    return [_pod("a", "blue"), _pod("b", "green"), _pod("c"),
            {"apiVersion": "v1", "kind": "Namespace", "metadata": {"name": "blue"}},
            _pod("d", "blue"), {"apiVersion": "v1", "kind": "ConfigMap"}, _pod("e", "green"), _pod("f", "blue")]


def all_codes_matrix(n, R):
    """Every code of the alphabet in every column, shifted per column so that rows mix codes."""
    v = np.zeros((n, R), dtype=np.uint8)
    for i in range(n):
        for r in range(R):
            v[i, r] = CODES[(i + r) % len(CODES)] if i < 2 * len(CODES) else CODES[(i * 5 + r * 3) % len(CODES)]
    return v


def numpy_counts(v, row_ns, G):
    out = np.zeros((G, v.shape[1], 6), dtype=np.uint32)
    for k, code in enumerate(FIELD_CODE):
        for g in range(G):
            out[g, :, k] = (v[row_ns == g] == code).sum(axis=0)
    return out


def test_symbols_exported():
    L = load()
    for name in ("kpe_corpus_num_namespaces", "kpe_corpus_namespace", "kpe_corpus_row_namespaces",
                 "kpe_corpus_namespace_rows", "kpe_fetch_namespace_counts", "kpe_namespace_counts_host",
                 "kpe_cli_summary_ns"):
        assert hasattr(L, name), name
    assert K.NS_COUNT_FIELDS == ("pass", "fail", "warn", "error", "skip", "undecided")
    assert callable(K.namespace_counts) and callable(K.cli_summary_ns) and callable(K.Engine.namespace_counts)


def test_groups_match_a_python_parse():
    docs = hand_corpus()
    c = K.Corpus(docs)
    names = c.namespaces
    want = [(d.get("metadata") or {}).get("namespace", "") for d in docs]
    got = [names[g] for g in c.row_namespaces()]
    assert got == want
    assert want[3] == "" and want[2] == "" and want[5] == ""  # the Namespace object groups under "", not "blue"
    assert len(set(names)) == len(names) and "" in names and {"blue", "green"} <= set(names)
    rows = c.namespace_rows()
    assert rows.dtype == np.uint64 and rows.sum() == c.n
    assert {names[g]: int(rows[g]) for g in range(len(names)) if rows[g]} == {"blue": 3, "green": 2, "": 3}
    assert load().kpe_corpus_namespace(c.h, len(names)) is None and load().kpe_corpus_namespace(c.h, -1) is None
    # "" exists even when every row has a namespace: a group without rows
    c2 = K.Corpus([_pod("a", "blue")])
    assert sorted(c2.namespaces) == ["", "blue"]
    assert c2.namespace_rows()[c2.namespaces.index("")] == 0 and c2.namespace_rows().sum() == 1
    # a line that is not a JSON object cannot become a row: the flattener refuses the batch
    with pytest.raises(K.KpeError) as e:
        K.Corpus((json.dumps(docs[0]) + "\n[1,2]\n").encode())
    assert e.value.status == KPE_E_INVALID


def test_group_invariants_on_synth():
    c = K.Corpus(K.synth_resources(0xC3, 700, mix=K.SYNTH_C3))
    names = c.namespaces
    assert len(set(names)) == len(names) and "" in names
    assert int(c.namespace_rows().sum()) == c.n
    assert np.array_equal(np.bincount(c.row_namespaces(), minlength=len(names)), c.namespace_rows().astype(np.int64))


def test_groups_do_not_move_the_digest():
    docs = hand_corpus()
    a, b = K.Corpus(docs), K.Corpus(docs)
    d = a.digest()
    a.namespaces, a.row_namespaces(), a.namespace_rows()
    assert a.digest() == d == b.digest()


def three_group_case():
    ps = K.PolicySet(copy.deepcopy(parity_policy_set()[:5]))
    # group = row % 3 and, past the first rows, code = f(row % 7): 21 consecutive rows put every
    # code into every group
    docs = [_pod(f"p{i}", ("blue", "green", None)[i % 3]) for i in range(len(CODES) * 8)]
    c = K.Corpus(docs)
    v = all_codes_matrix(c.n, ps.num_rules)
    for g in range(3):
        for r in range(ps.num_rules):  # every code in every column of every group
            assert set(v[c.row_namespaces() == g, r].tolist()) == set(CODES), (g, r)
    return ps, c, v


def test_host_fold_matches_numpy():
    ps, c, v = three_group_case()
    G, R = len(c.namespaces), ps.num_rules
    assert G == 3
    want = numpy_counts(v, c.row_namespaces(), G)
    got = K.namespace_counts(ps, c, v)
    assert got.shape == (G, R, 6) and got.dtype == np.uint32
    assert np.array_equal(got, want)
    assert (got > 0).all()
    # the six counters plus the derived NA are the group's rows
    na = np.stack([(v[c.row_namespaces() == g] == 0).sum(axis=0) for g in range(G)])
    assert np.array_equal(got.sum(axis=2) + na, np.broadcast_to(c.namespace_rows()[:, None], (G, R)))
    # windows: inner, the last group alone, no group
    assert np.array_equal(K.namespace_counts(ps, c, v, 1, 1), want[1:2])
    assert np.array_equal(K.namespace_counts(ps, c, v, G - 1), want[G - 1:])
    assert np.array_equal(K.namespace_counts(ps, c, v, 1), want[1:])
    assert K.namespace_counts(ps, c, v, 1, 0).shape == (0, R, 6)
    assert K.namespace_counts(ps, c, v, G, 0).shape == (0, R, 6)


def test_host_fold_writes_only_the_window():
    L = load()
    ps, c, v = three_group_case()
    G, R = len(c.namespaces), ps.num_rules
    want = numpy_counts(v, c.row_namespaces(), G)
    buf = np.full((G + 1, R, 6), SENTINEL, dtype=np.uint32)
    assert L.kpe_namespace_counts_host(ps.h, c.h, v.ctypes.data, 1, 2, buf.ctypes.data) == 0
    assert np.array_equal(buf[:2], want[1:3]) and (buf[2:] == SENTINEL).all()
    buf[:] = SENTINEL
    assert L.kpe_namespace_counts_host(ps.h, c.h, v.ctypes.data, 2, 0, buf.ctypes.data) == 0
    assert L.kpe_namespace_counts_host(ps.h, c.h, v.ctypes.data, 2, 0, None) == 0
    assert (buf == SENTINEL).all()


def test_argument_errors_without_device():
    L = load()
    ps, c, v = three_group_case()
    G, R = len(c.namespaces), ps.num_rules
    buf = np.full((G + 1, R, 6), SENTINEL, dtype=np.uint32)
    host = L.kpe_namespace_counts_host
    assert host(ps.h, c.h, v.ctypes.data, 0, G + 1, buf.ctypes.data) == KPE_E_INVALID
    assert host(ps.h, c.h, v.ctypes.data, G, 1, buf.ctypes.data) == KPE_E_INVALID
    assert host(ps.h, c.h, v.ctypes.data, G + 1, 0, buf.ctypes.data) == KPE_E_INVALID
    assert host(ps.h, c.h, v.ctypes.data, 1 << 63, 1 << 63, buf.ctypes.data) == KPE_E_INVALID
    assert host(None, c.h, v.ctypes.data, 0, G, buf.ctypes.data) == KPE_E_INVALID
    assert host(ps.h, None, v.ctypes.data, 0, G, buf.ctypes.data) == KPE_E_INVALID
    assert host(ps.h, c.h, None, 0, G, buf.ctypes.data) == KPE_E_INVALID
    assert host(ps.h, c.h, v.ctypes.data, 0, G, None) == KPE_E_INVALID
    # the device call checks its arguments before any device call: a fake handle is never read
    fetch = L.kpe_fetch_namespace_counts
    fake_dev = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    assert fetch(None, ps.h, c.h, 0, G, buf.ctypes.data) == KPE_E_INVALID
    assert fetch(fake_dev, None, c.h, 0, G, buf.ctypes.data) == KPE_E_INVALID
    assert fetch(fake_dev, ps.h, None, 0, G, buf.ctypes.data) == KPE_E_INVALID
    assert fetch(fake_dev, ps.h, c.h, 0, G, None) == KPE_E_INVALID
    assert fetch(fake_dev, ps.h, c.h, 0, G + 1, buf.ctypes.data) == KPE_E_INVALID
    assert fetch(fake_dev, ps.h, c.h, G, 1, buf.ctypes.data) == KPE_E_INVALID
    assert fetch(fake_dev, ps.h, c.h, 1, 0, buf.ctypes.data) == 0  # no group: nothing to do, nothing written
    assert (buf == SENTINEL).all()
    out = CliTotals()
    k = np.zeros((G, R, 6), dtype=np.uint32)
    assert L.kpe_cli_summary_ns(None, c.h, k.ctypes.data, 0, ctypes.byref(out)) == KPE_E_INVALID
    assert L.kpe_cli_summary_ns(ps.h, None, k.ctypes.data, 0, ctypes.byref(out)) == KPE_E_INVALID
    assert L.kpe_cli_summary_ns(ps.h, c.h, None, 0, ctypes.byref(out)) == KPE_E_INVALID
    assert L.kpe_cli_summary_ns(ps.h, c.h, k.ctypes.data, 0, None) == KPE_E_INVALID
    assert L.kpe_corpus_row_namespaces(None, buf.ctypes.data) == KPE_E_INVALID
    assert L.kpe_corpus_namespace_rows(c.h, None) == KPE_E_INVALID
    with pytest.raises(ValueError):
        K.namespace_counts(ps, c, v[:-1])
    with pytest.raises(ValueError):
        K.cli_summary_ns(ps, c, k[:-1])


# ---- kpe_cli_summary_ns against a restatement of the reference ----------------------------------

def go_wildcard(pattern, s):
    """github.com/IGLOU-EU/go-wildcard Match: '*' any run, '?' one rune; an empty pattern matches
    only the empty string."""
    if pattern == "":
        return s == ""
    rx = "".join(".*" if ch == "*" else "." if ch == "?" else re.escape(ch) for ch in pattern)
    return re.fullmatch(rx, s, re.S) is not None


_NAME_PART = re.compile(r"[A-Za-z0-9]([-A-Za-z0-9_.]*[A-Za-z0-9])?")
_DNS_LABEL = r"[a-z0-9]([-a-z0-9]*[a-z0-9])?"
_DNS_SUBDOMAIN = re.compile(_DNS_LABEL + r"(\." + _DNS_LABEL + r")*")


def _name_part_ok(s):
    return 0 < len(s) <= 63 and _NAME_PART.fullmatch(s) is not None


def _label_key_ok(k):  # validation.IsQualifiedName
    parts = k.split("/")
    if len(parts) == 1:
        return _name_part_ok(parts[0])
    if len(parts) != 2:
        return False
    return 0 < len(parts[0]) <= 253 and _DNS_SUBDOMAIN.fullmatch(parts[0]) is not None and _name_part_ok(parts[1])


def _label_value_ok(v):  # validation.IsValidLabelValue
    return v == "" or _name_part_ok(v)


def check_selector(sel, labels):
    """utils.CheckSelector (labels.go:10-24): nil -> false; wildcards.ReplaceInSelector; a
    selector LabelSelectorAsSelector cannot build -> false; Matches."""
    if sel is None:
        return False
    want = {}
    for k, v in (sel.get("matchLabels") or {}).items():
        if any(ch in k + v for ch in "*?"):
            hit = next(((k1, v1) for k1, v1 in sorted(labels.items()) if go_wildcard(k, k1) and go_wildcard(v, v1)), None)
            k, v = hit if hit else (re.sub(r"[*?]", "0", k), re.sub(r"[*?]", "0", v))
        want[k] = v
    exprs = sel.get("matchExpressions") or []
    for k, v in want.items():
        if not _label_key_ok(k) or not _label_value_ok(v):
            return False
    for e in exprs:
        vals = e.get("values") or []
        if not _label_key_ok(e.get("key", "")) or not all(_label_value_ok(x) for x in vals):
            return False
        if e.get("operator") in ("In", "NotIn"):
            if not vals:
                return False
        elif e.get("operator") in ("Exists", "DoesNotExist"):
            if vals:
                return False
        else:
            return False
    for k, v in want.items():
        if labels.get(k) != v:
            return False
    for e in exprs:
        op, has = e["operator"], e["key"] in labels
        isin = has and labels[e["key"]] in (e.get("values") or [])
        if (op == "In" and not isin) or (op == "NotIn" and isin) or (op == "Exists" and not has) or \
                (op == "DoesNotExist" and has):
            return False
    return True


def validation_failure_action(policy, ns, labels):
    """EngineResponse.GetValidationFailureAction (engineresponse.go:196-225)."""
    spec = policy.get("spec") or {}
    for o in spec.get("validationFailureActionOverrides") or []:
        action = o.get("action", "")
        if action not in ("audit", "enforce", "Audit", "Enforce"):
            continue
        nss = o.get("namespaces")  # absent or null: a nil slice; []: an empty one
        if nss is None:
            if check_selector(o.get("namespaceSelector"), labels):
                return action
        for pat in nss or []:
            if go_wildcard(pat, ns):
                if o.get("namespaceSelector") is None:
                    return action
                if check_selector(o.get("namespaceSelector"), labels):
                    return action
    return spec.get("validationFailureAction", "")


def reference_totals(policies, rule_names, verdicts, row_ns, ns_labels, audit_warn):
    """ResultCounts.addEngineResponse (result.go:34-68) per (resource, policy), the action from
    GetValidationFailureAction with the resource's namespace and that namespace's labels."""
    from oracle.report import _source_rule

    by_name = {p["metadata"]["name"]: p for p in policies}
    cols = {}
    for r, full in enumerate(rule_names):
        cols.setdefault(full.split("/", 1)[0], []).append(r)
    tot = {"pass": 0, "fail": 0, "warn": 0, "error": 0, "skip": 0}
    key = {1: "pass", 4: "error", 3: "warn", 5: "skip"}
    for i, row in enumerate(verdicts):
        for pname, rs in cols.items():
            pol = by_name[pname]
            responses = [(rule_names[r].split("/", 1)[1], int(row[r])) for r in rs if int(row[r]) in (1, 2, 3, 4, 5)]
            if not responses:
                continue
            scored = ((pol.get("metadata") or {}).get("annotations") or {}).get("policies.kyverno.io/scored") != "false"
            action = validation_failure_action(pol, row_ns[i], ns_labels.get(row_ns[i], {}))
            audit = action not in ("Enforce", "enforce")
            for r in rs:
                rname = rule_names[r].split("/", 1)[1]
                if not _source_rule(pol, rname).get("validate"):
                    continue
                for name, cell in responses:
                    if name != rname:
                        continue
                    if cell == 2:
                        tot["warn" if (not scored or (audit_warn and audit)) else "fail"] += 1
                    else:
                        tot[key[cell]] += 1
    return tot


def _variant(base, name, action, overrides=None, unscored=False):
    p = copy.deepcopy(base)
    p["metadata"]["name"] = name
    p["spec"]["validationFailureAction"] = action
    if overrides is not None:
        p["spec"]["validationFailureActionOverrides"] = overrides
    if unscored:
        p["metadata"].setdefault("annotations", {})["policies.kyverno.io/scored"] = "false"
    return p


PROD_SEL = {"matchLabels": {"env": "prod"}}

# name -> (spec.validationFailureAction, overrides, unscored)
OVERRIDE_CASES = {
    "enforce-on-prod": ("Audit", [{"action": "Enforce", "namespaces": ["team-*-prod"]}], False),
    "audit-on-prod": ("Enforce", [{"action": "Audit", "namespaces": ["team-*-prod"]}], False),
    "selector-only": ("Audit", [{"action": "Enforce", "namespaceSelector": PROD_SEL}], False),
    "selector-exprs": ("Enforce", [{"action": "audit", "namespaceSelector": {"matchExpressions": [
        {"key": "env", "operator": "In", "values": ["dev", "system"]},
        {"key": "tier", "operator": "DoesNotExist"}]}}], False),
    "selector-wild": ("Audit", [{"action": "enforce", "namespaceSelector": {"matchLabels": {"t?er": "g*"}}}], False),
    "selector-invalid": ("Audit", [{"action": "Enforce", "namespaceSelector": {"matchExpressions": [
        {"key": "env", "operator": "In", "values": []}]}}], False),
    "selector-null": ("Audit", [{"action": "Enforce", "namespaceSelector": None}], False),
    "globs-and-selector": ("Audit", [{"action": "Enforce", "namespaces": ["team-1*", "kube-*"],
                                      "namespaceSelector": PROD_SEL}], False),
    "invalid-action-first": ("Audit", [{"action": "Block", "namespaces": ["*"]},
                                       {"action": "Enforce", "namespaces": ["team-*-prod"]}], False),
    "first-wins": ("Audit", [{"action": "Audit", "namespaces": ["team-1*"]},
                             {"action": "Enforce", "namespaces": ["team-*"]}], False),
    "empty-namespaces": ("Audit", [{"action": "Enforce", "namespaces": [], "namespaceSelector": PROD_SEL}], False),
    "null-namespaces": ("Audit", [{"action": "Enforce", "namespaces": None, "namespaceSelector": PROD_SEL}], False),
    "unscored": ("Enforce", [{"action": "Audit", "namespaces": ["team-*-prod"]}], True),
    "cluster-scoped": ("Audit", [{"action": "Enforce", "namespaces": [""]}], False),
}


@pytest.fixture(scope="module")
def c3_case(oracle):
    """A few hundred SYNTH_C3 rows (namespaces team-<t>-prod / -dev, shop-<s>-prod, kube-system,
    default), a namespace label table over them, and the oracle's verdicts of the base policy."""
    nd = K.synth_resources(0xC3, 400, mix=K.SYNTH_C3)
    docs = [json.loads(x) for x in nd.split(b"\n") if x.strip()]
    row_ns = [(d.get("metadata") or {}).get("namespace", "") for d in docs]
    ns_labels = {}
    for ns in sorted(set(row_ns)):
        if ns.endswith("-prod"):
            ns_labels[ns] = {"env": "prod", "tier": "gold" if ns.startswith("team-1") else "bronze"}
        elif ns.endswith("-dev"):
            ns_labels[ns] = {"env": "dev"}
        elif ns == "kube-system":
            ns_labels[ns] = {"env": "system", "tier": "gold"}
    assert any(re.fullmatch(r"team-\d+-prod", ns) for ns in row_ns) and "default" in row_ns
    base = parity_policy_set()[0]
    return nd, row_ns, ns_labels, base


def _totals_for(oracle, case, pols):
    nd, row_ns, ns_labels, _ = case
    ps = K.PolicySet(pols)
    names = oracle.rule_names(pols)
    assert ps.rule_names == names
    v = oracle.validate(pols, nd, ns_labels=ns_labels, nthreads=4)
    corpus = K.Corpus(nd, ns_labels)
    assert [corpus.namespaces[g] for g in corpus.row_namespaces()] == row_ns
    table = K.namespace_counts(ps, corpus, v)
    return ps, corpus, v, names, table


@pytest.mark.parametrize("name", sorted(OVERRIDE_CASES))
def test_cli_summary_ns_overrides_match_the_reference(oracle, c3_case, name):
    nd, row_ns, ns_labels, base = c3_case
    action, overrides, unscored = OVERRIDE_CASES[name]
    pol = _variant(base, name, action, overrides, unscored)
    plain = _variant(base, name, action, None, unscored)
    ps, corpus, v, names, table = _totals_for(oracle, c3_case, [pol])
    assert (v == 2).any()
    differs = False
    for aw in (False, True):
        want = reference_totals([pol], names, v, row_ns, ns_labels, aw)
        got = K.cli_summary_ns(ps, corpus, table, aw)
        assert got == want, (name, aw)
        no_override = reference_totals([plain], names, v, row_ns, ns_labels, aw)
        differs |= want != no_override
        if not aw:  # the action only matters under --audit-warn
            assert want == no_override
    # overrides that can never apply (or an unscored policy, whose fails are warns anyway) leave
    # the totals alone; the plain glob cases must move them, or the test shows nothing
    if name in ("empty-namespaces", "selector-invalid", "selector-null", "unscored"):
        assert not differs, name
    if name in ("enforce-on-prod", "audit-on-prod", "invalid-action-first", "null-namespaces", "selector-only"):
        assert differs, name


def test_cli_summary_ns_several_policies(oracle, c3_case):
    """Every case as one policy set (per-policy actions within one group), with a second base
    policy and a policy whose rules share a name (name_mult)."""
    nd, row_ns, ns_labels, base = c3_case
    pols = [_variant(base, n, a, o, u) for n, (a, o, u) in sorted(OVERRIDE_CASES.items())]
    other = parity_policy_set()[1]
    pols.append(_variant(other, "other-enforced", "Enforce", [{"action": "Audit", "namespaces": ["default"]}]))
    dup = _variant(other, "dup-names", "Audit", [{"action": "Enforce", "namespaces": ["kube-*", "team-2*"]}])
    dup["spec"]["rules"].append(copy.deepcopy(dup["spec"]["rules"][0]))
    pols.append(dup)
    ps, corpus, v, names, table = _totals_for(oracle, c3_case, pols)
    plain = copy.deepcopy(pols)
    for p in plain:
        p["spec"].pop("validationFailureActionOverrides", None)
    for aw in (False, True):
        want = reference_totals(pols, names, v, row_ns, ns_labels, aw)
        assert K.cli_summary_ns(ps, corpus, table, aw) == want
        assert want["fail"] > 0 and want["warn"] > 0
        if aw:
            assert want != reference_totals(plain, names, v, row_ns, ns_labels, aw)
    with pytest.raises(K.KpeError):  # the per-rule totals cannot answer it
        K.cli_summary(ps, _rule_counts(table), audit_warn=True)


def _rule_counts(table):
    s = table.sum(axis=0, dtype=np.uint64)
    return [dict(zip(K.NS_COUNT_FIELDS, (int(x) for x in s[r])), na=0) for r in range(s.shape[0])]


def test_without_overrides_equals_cli_summary(oracle, c3_case):
    nd, row_ns, ns_labels, base = c3_case
    pols = [_variant(base, "plain-audit", "Audit"), _variant(base, "plain-enforce", "Enforce"),
            _variant(parity_policy_set()[1], "plain-unscored", "Enforce", unscored=True)]
    ps, corpus, v, names, table = _totals_for(oracle, c3_case, pols)
    from oracle import report as oracle_report

    for aw in (False, True):
        want = K.cli_summary(ps, _rule_counts(table), aw)
        assert K.cli_summary_ns(ps, corpus, table, aw) == want
        assert want == oracle_report.cli_summary(pols, names, v, aw)
    assert K.cli_summary(ps, _rule_counts(table), True) != K.cli_summary(ps, _rule_counts(table), False)


def test_merge_namespace_counts(oracle, c3_case):
    nd, row_ns, ns_labels, base = c3_case
    pols = [base, parity_policy_set()[1]]
    ps = K.PolicySet(pols)
    v = oracle.validate(pols, nd, nthreads=4)
    lines = [x for x in nd.split(b"\n") if x.strip()]
    cut = len(lines) // 2 + 3
    whole = K.Corpus(nd)
    parts = []
    for a, b in ((0, cut), (cut, len(lines))):
        c = K.Corpus(b"\n".join(lines[a:b]))
        parts.append((c.namespaces, K.namespace_counts(ps, c, v[a:b])))
    assert parts[0][0] != parts[1][0]  # each shard numbers its groups itself
    names, merged = merge_namespace_counts(parts)
    assert merged.dtype == np.uint64 and len(set(names)) == len(names)
    want = dict(zip(whole.namespaces, K.namespace_counts(ps, whole, v)))
    got = dict(zip(names, merged))
    for nm in set(want) | set(got):
        a = want.get(nm, np.zeros((ps.num_rules, 6), np.uint32))
        b = got.get(nm, np.zeros((ps.num_rules, 6), np.uint64))
        assert np.array_equal(a.astype(np.uint64), b), nm
    assert merged.sum() == int((v != 0).sum()) - int((v == 6).sum())
    assert merge_namespace_counts([])[0] == []
    with pytest.raises(ValueError):
        merge_namespace_counts([(["a"], np.zeros((2, 3, 6), np.uint32))])
