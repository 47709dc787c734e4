"""Incremental background scans keyed by the resource hash.

The background controller (pkg/controllers/report/background/controller.go:247-297,
needsReconcile) rescans a resource when its CalculateResourceHash
(pkg/utils/report/metadata.go:137-155) differs from the hash recorded on its report, when a
policy or exception resourceVersion changed, or when the last scan is older than the forced
rescan interval. BackgroundScanner keeps the last verdict row of every resource: a scan
re-flattens and re-evaluates only the rows that are new or whose hash changed, and every row
when the policy set, the namespace labels or `force` say so. The hash is computed by
kpe_resource_hashes (C++, 16 threads); the evaluation is the device path (kpe_evaluate).
"""
import ctypes
import json

import numpy as np

from ._lib import KpeError, load
from .engine import SEL, Corpus, rule_salts


def resource_hash(resource) -> str:
    """CalculateResourceHash of one resource (a dict or its JSON text)."""
    raw = resource if isinstance(resource, bytes) else (
        resource.encode() if isinstance(resource, str) else json.dumps(resource).encode())
    out = ctypes.create_string_buffer(33)
    st = load().kpe_resource_hash(raw, len(raw), out)
    if st != 0:
        raise KpeError(st, "resource is not a JSON object")
    return out.value.decode()


NO_HASH = "-" * 32  # kpe_resource_hashes' mark of a row that is not a JSON object


def resource_hashes(ndjson: bytes):
    """CalculateResourceHash of every NDJSON row (the rows kpe_corpus_flatten makes); NO_HASH
    for a row that is not a JSON object."""
    L = load()
    n = L.kpe_resource_hashes(ndjson, len(ndjson), None, 0)
    buf = ctypes.create_string_buffer(max(n, 1) * 32)
    m = L.kpe_resource_hashes(ndjson, len(ndjson), buf, n)
    if m < 0:
        raise KpeError(-m, "resource hash buffer")
    raw = buf.raw
    return [raw[32 * i:32 * i + 32].decode() for i in range(m)]


def ndjson_rows(ndjson: bytes):
    """The non-blank NDJSON lines, trimmed as the flattener trims them (flatten.cpp flatten_range)."""
    rows = []
    for line in ndjson.split(b"\n"):
        t = line.strip(b" \t\r")
        if t:
            rows.append(t)
    return rows


def _key(row: bytes, i: int):
    """Report identity of a resource: its UID when set, else (apiVersion, kind, namespace, name);
    a row that is not a JSON object is keyed by its position (it is re-evaluated every scan)."""
    try:
        d = json.loads(row)
    except ValueError:
        d = None
    if not isinstance(d, dict):
        return ("row", i)
    meta = d.get("metadata") if isinstance(d.get("metadata"), dict) else {}
    uid = meta.get("uid")
    if isinstance(uid, str) and uid:
        return ("uid", uid)
    return (d.get("apiVersion"), d.get("kind"), meta.get("namespace"), meta.get("name"))


class BackgroundScanner:
    """Verdict rows of the last scan per resource; `scan` evaluates what changed."""

    def __init__(self, engine):
        self.engine = engine
        self._rows = {}  # key -> (hash, verdict row)
        self._policy_token = None
        self._policies = None  # the PolicySet of the last scan (held: identity is the default token)
        self._nrules = None
        self._ns_labels = None
        self.last_stats = {}

    def scan(self, policies, ndjson: bytes, ns_labels=None, policy_version=None, force=False):
        """Verdict matrix (N x R) of the corpus in row order. `policy_version` stands for the
        policies' and exceptions' resourceVersions (any change rescans every row); by default
        the PolicySet object itself."""
        rows = ndjson_rows(ndjson)
        hashes = resource_hashes(b"\n".join(rows))
        keys = [_key(r, i) for i, r in enumerate(rows)]
        R = policies.num_rules
        if policy_version is not None:
            same_policies = policy_version == self._policy_token
        else:  # the PolicySet itself: compared by identity while this scanner holds it
            same_policies = self._policy_token is None and policies is self._policies
        full = force or not same_policies or R != self._nrules or ns_labels != self._ns_labels
        dirty = [i for i, (k, h) in enumerate(zip(keys, hashes))
                 if full or h == NO_HASH or k not in self._rows or self._rows[k][0] != h]
        out = np.zeros((len(rows), R), dtype=np.uint8)
        if dirty:
            delta = b"\n".join(rows[i] for i in dirty)
            nsl = json.dumps(ns_labels).encode() if isinstance(ns_labels, dict) else ns_labels
            v, _, _ = self.engine.evaluate(policies, Corpus(delta, nsl))
            out[dirty] = v
        fresh = set(dirty)
        rows_next = {}
        for i, (k, h) in enumerate(zip(keys, hashes)):
            if i not in fresh:
                out[i] = self._rows[k][1]
            rows_next[k] = (h, out[i].copy())
        self._rows = rows_next  # resources absent from this scan are forgotten (deleted)
        self._policy_token, self._ns_labels = policy_version, ns_labels
        self._policies, self._nrules = policies, R
        self.last_stats = {"rows": len(rows), "rescanned": len(dirty), "full": bool(full)}
        return out


class ResidentScanner:
    """One corpus resident on the device, re-evaluated when the policies change; `apply` returns
    only the rows whose report changes.

    The background controller re-evaluates every resource after a policy or PolicyException change
    and writes a report only when it differs from the stored one (pkg/controllers/report/
    background/controller.go:379-419,463; ReportsAreIdentical, pkg/controllers/report/utils/
    utils.go:66-88). Here the last result stays on the device (Engine.keep_results, or with
    keep="fingerprints" Engine.keep_fingerprints) and the comparison runs there (Engine.changed_rows,
    Engine.changed_rows_fp): the unchanged rows never cross to the host."""

    MESSAGE_CODES = SEL(2) | SEL(4) | SEL(5)  # FAIL, ERROR, SKIP: results whose message the policy text decides

    def __init__(self, engine, ndjson: bytes, ns_labels=None, keep="matrix", fingerprints=None, edits=None,
                 reports=False):
        """reports=True: the scanner keeps the NDJSON lines and evaluates with check masks, so that
        `reports(rows)` can render the PolicyReport results of rows of the last applied PolicySet.

        keep="matrix" (the default): the last verdict matrix stays on the device (N x R bytes) and
        the comparison is exact. keep="fingerprints": 8 bytes per row stay (Engine.keep_fingerprints;
        two different result sets of a row collide with probability 2^-64), they do not depend on
        the rule order, and they can be saved (`fingerprints()`, `edits`) and given back
        (`fingerprints=`, `edits=`) to a scanner over a re-uploaded corpus or in a new process: its
        first `apply` then returns only the rows that really changed."""
        if keep not in ("matrix", "fingerprints"):
            raise ValueError('keep: "matrix" or "fingerprints"')
        if keep != "fingerprints" and (fingerprints is not None or edits is not None):
            raise ValueError('fingerprints, edits: only with keep="fingerprints"')
        self.engine = engine
        self.keep = keep
        nsl = json.dumps(ns_labels).encode() if isinstance(ns_labels, dict) else ns_labels
        self.corpus = Corpus(ndjson, nsl).upload(engine.device)
        self._policies = None  # the PolicySet of the kept result (held while its matrix is kept)
        self._with_reports = bool(reports)
        self._lines = ndjson_rows(ndjson) if reports else None  # row i of the corpus is line i
        self._applied = None  # the PolicySet of the last apply (what `reports` renders)
        self.edits = dict(edits or {})  # policy name -> edits seen (keep="fingerprints": folded into msg_salts)
        if fingerprints is not None:
            engine.load_fingerprints(self.corpus, fingerprints)
        self.last_stats = {}

    def fingerprints(self):
        """keep="fingerprints": the kept fingerprints, one uint64 per row (None before the first
        apply): what a caller stores with the reports, together with `edits`."""
        return self.engine.kept_fingerprints(self.corpus) if self.keep == "fingerprints" else None

    def _apply_fp(self, policies, edited):
        eng, corpus = self.engine, self.corpus
        for name in set(edited):
            self.edits[name] = self.edits.get(name, 0) + 1
        msg = rule_salts(policies)
        for r, n in enumerate(policies.rule_names):
            msg[r] ^= np.uint64(self.edits.get(n.split("/", 1)[0], 0))
        eng.evaluate_async(policies, corpus, masks=self._with_reports)
        self._applied = policies
        if eng.kept_fingerprints(corpus, 0, 0) is None:
            # nothing to compare with: against "no report" (fingerprint 0), every row that has a response
            eng.load_fingerprints(corpus, np.zeros(corpus.n, dtype=np.uint64))
        rows, vr, _, total = eng.changed_rows_fp(policies, corpus, msg_salts=msg, msg_codes=self.MESSAGE_CODES)
        eng.keep_fingerprints(policies, corpus, msg_salts=msg, msg_codes=self.MESSAGE_CODES)
        self.last_stats = {"rows": corpus.n, "changed": total}
        return {int(i): vr[k].copy() for k, i in enumerate(rows)}

    def apply(self, policies, edited=()):
        """Evaluate `policies` (a PolicySet) on the corpus and return {row: verdict row} of the rows
        that differ from the last apply; the first call returns every row that has a response.
        Rules are paired by "<policy>/<rule>" name. `edited` names policies whose text changed
        under the same name: their FAIL / ERROR / SKIP cells count as changed whatever they were,
        since the message may differ under an equal verdict."""
        if self.keep == "fingerprints":
            return self._apply_fp(policies, edited)
        eng, corpus = self.engine, self.corpus
        eng.evaluate_async(policies, corpus, masks=self._with_reports)
        self._applied = policies
        if self._policies is None:
            v, _, _ = eng.fetch(policies, corpus)  # nothing to compare with: the whole matrix, once
            out = {int(i): v[i].copy() for i in np.flatnonzero((v != 0).any(axis=1))}
            total = len(out)
        else:
            names = set(edited)
            always = np.array([self.MESSAGE_CODES if n.split("/", 1)[0] in names else 0 for n in policies.rule_names],
                              dtype=np.uint8)
            rows, vr, total = eng.changed_rows(policies, corpus, always=always)
            out = {int(i): vr[k].copy() for k, i in enumerate(rows)}
        eng.keep_results(policies, corpus)
        self._policies = policies
        self.last_stats = {"rows": corpus.n, "changed": total}
        return out

    def reports(self, rows):
        """{row: PolicyReport results} of the listed rows under the last applied PolicySet, with
        messages (Engine.report_rows: one sparse fetch of what the rows' entries need, one bulk
        render). Needs reports=True; typically called with the rows `apply` returned."""
        if not self._with_reports:
            raise KpeError(5, "ResidentScanner(reports=True) keeps what reports() needs")  # KPE_E_STATE
        if self._applied is None:
            raise KpeError(5, "no apply yet")
        rows = [int(i) for i in rows]
        res = self.engine.report_rows(self._applied, self.corpus, rows, resources=[self._lines[i] for i in rows])
        return dict(zip(rows, res))
