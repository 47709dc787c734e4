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


def namespace_label_events(upserts=(), deleted=()):
    """The namespace label events among resource events (ResidentScanner(ns_objects=True)), as a
    patch for set_namespace_labels: {name: labels, or None to remove the entry}. upserts: NDJSON
    lines (or parsed resources); an `apiVersion: v1, kind: Namespace` object sets the entry of its
    metadata.name to its string-valued metadata.labels. deleted: the deleted resources, as lines,
    parsed resources or (apiVersion, kind, namespace, name) keys; a Namespace among them removes
    its entry. Deletes count after upserts; a later event of a name replaces an earlier one. No
    device, no library."""
    def parsed(x):
        if isinstance(x, (bytes, bytearray, str)):
            try:
                x = json.loads(x)
            except ValueError:
                return None
        return x if isinstance(x, dict) else None

    def ns_name(d):
        if d is None or d.get("apiVersion") != "v1" or d.get("kind") != "Namespace":
            return None
        meta = d.get("metadata") if isinstance(d.get("metadata"), dict) else {}
        name = meta.get("name")
        return name if isinstance(name, str) and name else None

    out = {}
    for u in upserts:
        d = parsed(u)
        name = ns_name(d)
        if name is not None:
            labels = d["metadata"].get("labels")
            out[name] = {k: v for k, v in labels.items() if isinstance(v, str)} if isinstance(labels, dict) else {}
    for x in deleted:
        if isinstance(x, tuple):
            name = x[3] if len(x) == 4 and x[0] == "v1" and x[1] == "Namespace" and isinstance(x[3], str) and x[3] else None
        else:
            name = ns_name(parsed(x))
        if name is not None:
            out[name] = None
    return out


class RowMap:
    """Bookkeeping of a resident corpus under resource churn; no device, no library.

    Resources live in segments (corpora): segment 0 is the corpus the scanner was built over, every
    `update` that flattens something appends one. A resource has a logical row for life: the
    initial rows are 0..n-1, new resources are appended, a deleted resource's index is never
    reused. A replaced or deleted resource's physical row is retired in its segment. The map
    holds logical row -> (segment, row), its inverse per segment, key -> logical row and the
    resource hash per logical row.

    Compaction (one segment again, live rows in logical order) is due past `max_segments`
    segments or once more than `max_retired` of the physical rows are retired."""

    def __init__(self, keys, hashes, max_segments=16, max_retired=0.25):
        keys, hashes = list(keys), list(hashes)
        if len(keys) != len(hashes):
            raise ValueError("one hash per key")
        self.max_segments, self.max_retired = int(max_segments), float(max_retired)
        self.loc = [(0, i) for i in range(len(keys))]  # logical row -> (segment, row), None: deleted
        self.back = [list(range(len(keys)))]  # per segment: row -> logical row, -1: retired
        self.hashes = hashes  # per logical row (None: deleted)
        self.keys = keys
        self.index = {k: i for i, k in enumerate(keys)}  # a key that occurs twice names its last row
        self.retired = 0

    @property
    def n_logical(self):
        return len(self.loc)

    @property
    def n_physical(self):
        return sum(len(b) for b in self.back)

    @property
    def n_live(self):
        return self.n_physical - self.retired

    @property
    def segments(self):
        return len(self.back)

    def live(self):
        """The live logical rows, ascending."""
        return [i for i, p in enumerate(self.loc) if p is not None]

    def row_of(self, key_or_row):
        """The live logical row a key or a logical row names, or None."""
        if isinstance(key_or_row, (int, np.integer)) and not isinstance(key_or_row, bool):
            i = int(key_or_row)
            return i if 0 <= i < len(self.loc) and self.loc[i] is not None else None
        return self.index.get(key_or_row)

    def plan(self, upserts, deletes=()):
        """What an update does, without doing it. upserts: (key, hash) per offered resource;
        deletes: keys or logical rows. Returns a dict: `items`, a list of (offered index, logical
        row or None for a new resource) to flatten, in offered order; `skipped`, the offered
        resources whose hash equals the stored one; `deletes`, the logical rows to delete,
        ascending. A key offered twice counts once, by its last occurrence; a resource both
        offered and deleted is deleted. NO_HASH never equals a stored hash."""
        dele = sorted({r for r in (self.row_of(d) for d in deletes) if r is not None})
        dead = set(dele)
        last = {}
        for i, (k, _) in enumerate(upserts):
            last[k] = i
        items, skipped = [], 0
        for i, (k, h) in enumerate(upserts):
            if last[k] != i:
                continue
            l = self.index.get(k)
            if l is not None and l in dead:
                continue
            if l is not None and h != NO_HASH and self.hashes[l] == h:
                skipped += 1
                continue
            items.append((i, l))
        return {"items": items, "skipped": skipped, "deletes": dele, "upserts": list(upserts)}

    def _retire(self, l, out):
        s, r = self.loc[l]
        self.back[s][r] = -1
        self.retired += 1
        out.setdefault(s, []).append(r)

    def commit(self, plan):
        """Apply a plan: its items become the rows of a new segment, in order. Returns (the new
        segment or None when nothing was flattened, the logical row of each item, {segment:
        rows to retire there})."""
        retire, rows = {}, []
        seg = len(self.back) if plan["items"] else None
        if seg is not None:
            self.back.append([])
        for j, (i, l) in enumerate(plan["items"]):
            k, h = plan["upserts"][i]
            if l is None:
                l = len(self.loc)
                self.loc.append(None)
                self.hashes.append(None)
                self.keys.append(k)
                self.index[k] = l
            else:
                self._retire(l, retire)
            self.loc[l], self.hashes[l] = (seg, j), h
            self.back[seg].append(l)
            rows.append(l)
        for l in plan["deletes"]:
            self._retire(l, retire)
            self.loc[l], self.hashes[l] = None, None
            if self.index.get(self.keys[l]) == l:
                del self.index[self.keys[l]]
        return seg, rows, retire

    def translate(self, seg, rows):
        """(position in rows, logical row) of the rows of a segment's row list that are live; rows
        of retired physical rows are dropped: their resource lives elsewhere, or nowhere."""
        b = self.back[seg]
        return [(k, b[int(r)]) for k, r in enumerate(rows) if b[int(r)] >= 0]

    def group(self, rows):
        """{segment: [(logical row, row)]} of live logical rows, in the order given."""
        out = {}
        for l in rows:
            p = self.loc[int(l)]
            if p is not None:
                out.setdefault(p[0], []).append((int(l), p[1]))
        return out

    def needs_compaction(self):
        return self.segments > self.max_segments or self.retired > self.max_retired * self.n_physical

    def compact(self):
        """One segment again: the live logical rows, ascending, become its rows 0..m-1. Logical
        indices do not move. Returns the live rows."""
        live = self.live()
        for j, l in enumerate(live):
            self.loc[l] = (0, j)
        self.back = [list(live)]
        self.retired = 0
        return live


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
    Engine.changed_rows_fp): the unchanged rows never cross to the host.

    With keyed=True the corpus also follows resource events (controller.go:247-297): `update`
    flattens only the resources whose hash changed into a delta segment, compares them on the device
    with the kept rows they replace and retires those rows where they were; the corpus, its upload
    and its kept results stay. Rows are then logical rows (RowMap).

    Namespace label changes (controller.go:310-318 reads the labels fresh at every rescan) are
    applied in place too: `set_namespace_labels` replaces the label table of every segment on the
    device and returns the rows whose report changes; with ns_objects=True `update` reads them off
    the Namespace objects among its events.

    One policy edited, added or removed out of many (controller.go:379-419 keeps the stored results
    of unchanged policies): `apply_edit` evaluates the edited policies alone and splices their
    columns into the kept matrix (Engine.splice_results), keep="matrix" only."""

    MESSAGE_CODES = SEL(2) | SEL(4) | SEL(5)  # FAIL, ERROR, SKIP: results whose message the policy text decides

    def __init__(self, engine, ndjson: bytes, ns_labels=None, keep="matrix", fingerprints=None, edits=None,
                 reports=False, keyed=False, max_segments=16, max_retired=0.25, ns_objects=False):
        """keyed=True: the scanner also follows resource churn (`update`, `compact`, `matrix`). It
        then keeps the NDJSON lines, the resource-key index and the per-row resource hash
        (`resource_hashes`), and holds the corpus as segments (RowMap). `update` compacts past
        max_segments segments or once more than max_retired of the physical rows are retired; both
        defaults are unmeasured guesses (every segment adds launches to an `apply`, every retired
        row is scanned for nothing), not tuned values. Without keyed the class is what it was.

        ns_objects=True (with keyed): `update` treats `apiVersion: v1, kind: Namespace` upserts and
        deletes as label events of metadata.name (namespace_label_events) and applies them with
        `set_namespace_labels` before it flattens the delta segment.

        reports=True: the scanner keeps the NDJSON lines and evaluates with check masks, so that
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
        if ns_objects and not keyed:
            raise ValueError("ns_objects: only with keyed=True")
        self.engine = engine
        self.keep = keep
        nsl = json.dumps(ns_labels).encode() if isinstance(ns_labels, dict) else ns_labels
        self._nsl = nsl
        self.corpus = Corpus(ndjson, nsl).upload(engine.device)
        self._policies = None  # the PolicySet of the kept result (held while its matrix is kept)
        self._with_reports = bool(reports)
        self._keyed = bool(keyed)
        self._ns_objects = bool(ns_objects)
        self._stale = False  # keyed: rows were retired since the segments' last evaluation
        self._unevaluated = False  # keyed: the segment was gathered (compact) and not evaluated since
        self._lines = ndjson_rows(ndjson) if (reports or keyed) else None  # logical row i is line i
        self._segs = [self.corpus]  # keyed: the segments (RowMap); segment 0 is self.corpus
        self._map = None
        self._updated = False
        self._msg = None  # keep="fingerprints": the msg_salts of the last apply
        if keyed:
            if len(self._lines) != self.corpus.n:
                raise KpeError(2, "keyed: one NDJSON line per corpus row")  # KPE_E_INVALID
            self._map = RowMap([_key(r, i) for i, r in enumerate(self._lines)],
                               resource_hashes(b"\n".join(self._lines)), max_segments, max_retired)
        self._applied_v = None  # the PolicySet of the last apply (what `reports` renders), or after an
        # apply_edit a callable that makes it (see the _applied property)
        self._edit = None  # the partial PolicySet of an apply_edit, while the segments' last evaluation is of it
        self._edit_ok = False  # reports(policies="edited") may render from it: nothing happened since
        self.edits = dict(edits or {})  # policy name -> edits seen (keep="fingerprints": folded into msg_salts)
        if fingerprints is not None:
            engine.load_fingerprints(self.corpus, fingerprints)
        self.last_stats = {}

    @property
    def _applied(self):
        """The PolicySet of the last apply. After apply_edit(full, ...) with a callable `full` it
        is made (compiled) here, by the first reader that needs the whole set."""
        a = self._applied_v
        if a is not None and callable(a):
            a = self._applied_v = a()
            if self._policies is not None:
                self._policies = a
        return a

    @_applied.setter
    def _applied(self, ps):
        self._applied_v = ps

    @property
    def resource_hashes(self):
        """keyed: CalculateResourceHash per logical row (None for a deleted resource)."""
        return None if self._map is None else list(self._map.hashes)

    def fingerprints(self):
        """keep="fingerprints": the kept fingerprints, one uint64 per row (None before the first
        apply): what a caller stores with the reports, together with `edits`. Once an `update` has
        happened: (rows, fps), the live logical rows and one value for each."""
        if self.keep != "fingerprints":
            return None
        if not self._updated:
            return self.engine.kept_fingerprints(self.corpus)
        if self.engine.kept_fingerprints(self._segs[0], 0, 0) is None:
            return None
        live = np.array(self._map.live(), dtype=np.uint64)
        return live, self._fps_by_row()[live.astype(np.int64)]

    def _fps_by_row(self):
        """The kept fingerprints by logical row (0 where nothing is kept, or nothing lives)."""
        out = np.zeros(self._map.n_logical, dtype=np.uint64)
        for s, seg in enumerate(self._segs):
            fp = self.engine.kept_fingerprints(seg)
            if fp is None:
                continue
            back = np.array(self._map.back[s], dtype=np.int64)
            out[back[back >= 0]] = fp[back >= 0]
        return out

    def _apply_fp(self, policies, edited):
        eng, corpus = self.engine, self.corpus
        for name in set(edited):
            self.edits[name] = self.edits.get(name, 0) + 1
        msg = rule_salts(policies)
        for r, n in enumerate(policies.rule_names):
            msg[r] ^= np.uint64(self.edits.get(n.split("/", 1)[0], 0))
        self._msg = msg
        if self._keyed:
            return self._apply_segments(policies, None, msg)
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
        if self._keyed:
            names = set(edited)
            return self._apply_segments(policies, np.array(
                [self.MESSAGE_CODES if n.split("/", 1)[0] in names else 0 for n in policies.rule_names], dtype=np.uint8), None)
        eng.evaluate_async(policies, corpus, masks=self._with_reports)
        self._applied = policies
        self._stale, self._edit = False, None
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

    # ---- namespace label changes ----
    def set_namespace_labels(self, labels, replace=False):
        """The labels of namespaces changed (background/controller.go:310-318 reads them fresh at
        every rescan): labels is {namespace: {key: value}, or None to remove the entry}, a patch by
        default, the whole table with replace=True (Engine.set_namespace_labels). The table of every
        segment is replaced in place, on the device; the corpus, its upload, the kept results and
        the retired rows stay, later delta segments flatten with the new table and `compact` carries it.

        With a PolicySet applied, returns {row: verdict row} of exactly the rows whose report
        changes: the segments are evaluated again and compared with the kept result as `apply`
        compares them with edited=() (keep="fingerprints": under the same message salts; `edits`
        is untouched), and that result is then kept. {} before the first `apply`. When no entry
        really changes nothing is done on the device."""
        eng = self.engine
        relabelled = max(eng.set_namespace_labels(seg, labels, replace) for seg in self._segs)
        stats = {"relabelled": relabelled, "changed": 0}
        out = {}
        if relabelled:
            self._nsl = json.dumps(self._segs[0].namespace_labels()).encode()
            ps = self._applied
            if ps is not None and self._keyed:
                out = self._apply_segments(ps, np.zeros(ps.num_rules, dtype=np.uint8) if self._msg is None else None,
                                           self._msg)
                stats.update(rows=self.last_stats["rows"], segments=self.last_stats["segments"])
            elif ps is not None:
                stats["rows"] = self.corpus.n
                eng.evaluate_async(ps, self.corpus, masks=self._with_reports)
                self._stale, self._edit = False, None
                if self.keep == "fingerprints":
                    rows, vr, _, _ = eng.changed_rows_fp(ps, self.corpus, msg_salts=self._msg, msg_codes=self.MESSAGE_CODES)
                else:
                    rows, vr, _ = eng.changed_rows(ps, self.corpus)
                self._keep(self.corpus)
                out = {int(i): vr[k].copy() for k, i in enumerate(rows)}
            stats["changed"] = len(out)
        self.last_stats = stats
        return out

    def _refresh(self):
        """Evaluate the segments again when rows were retired since their last evaluation: a
        retired row gives no response from the next evaluation on."""
        if self._applied_v is None:
            raise KpeError(5, "no apply yet")  # KPE_E_STATE
        if self._stale:
            self.engine.evaluate_batch_async(self._applied, self._segs, masks=self._with_reports)
            self._stale, self._edit, self._unevaluated = False, None, False

    def namespace_counts(self):
        """Per-namespace rule counts of the resident corpus under the last applied PolicySet:
        (names, (G, R, 6) uint64 counts, last axis NS_COUNT_FIELDS). Every segment's table is
        reduced on its device (Engine.namespace_counts) and the tables are merged by namespace name
        on the host (shard.merge_namespace_counts: a delta segment has few groups). Retired rows
        give no response and count nowhere."""
        from .shard import merge_namespace_counts

        self._refresh()
        return merge_namespace_counts([(seg.namespaces, self.engine.namespace_counts(self._applied, seg))
                                       for seg in self._segs])

    def cli_summary(self, audit_warn=False):
        """`kyverno apply` totals of the resident corpus under the last applied PolicySet, the
        action resolved per namespace from the current labels (cli_summary_ns per segment, summed)."""
        from .engine import cli_summary_ns

        self._refresh()
        out = {"pass": 0, "fail": 0, "warn": 0, "error": 0, "skip": 0}
        for seg in self._segs:
            t = cli_summary_ns(self._applied, seg, self.engine.namespace_counts(self._applied, seg), audit_warn)
            for k in out:
                out[k] += t[k]
        return out

    def reports(self, rows, policies=None):
        """{row: PolicyReport results} of the listed rows under the last applied PolicySet, with
        messages (Engine.report_rows: one sparse fetch of what the rows' entries need, one bulk
        render). Needs reports=True; typically called with the rows `apply` returned.

        policies="edited", right after an `apply_edit`: only the entries of the edited and added
        policies, rendered from the partial evaluation; what a consumer swaps into the stored
        report, as the background controller does (controller.go:379-419). KPE_E_STATE once
        anything else happened. The default evaluates the full set first when the last evaluation
        was a partial one."""
        if not self._with_reports:
            raise KpeError(5, "ResidentScanner(reports=True) keeps what reports() needs")  # KPE_E_STATE
        if self._applied_v is None:
            raise KpeError(5, "no apply yet")
        if policies not in (None, "edited"):
            raise ValueError('policies: None or "edited"')
        if policies == "edited":
            if self._edit is None or not self._edit_ok:
                raise KpeError(5, 'reports(policies="edited"): only right after an apply_edit')
            ps = self._edit
        else:
            if self._edit is not None or self._unevaluated:  # the last evaluation is of the edited policies alone, or none
                self._refresh()
            ps = self._applied
        rows = [int(i) for i in rows]
        if not ps.num_rules:
            return {i: [] for i in rows}
        if not self._keyed:
            res = self.engine.report_rows(ps, self.corpus, rows, resources=[self._lines[i] for i in rows])
            return dict(zip(rows, res))
        out = {i: [] for i in rows}  # a deleted resource has no report
        for s, pr in self._map.group(rows).items():
            res = self.engine.report_rows(ps, self._segs[s], [r for _, r in pr],
                                          resources=[self._lines[l] for l, _ in pr])
            out.update(zip((l for l, _ in pr), res))
        return out

    # ---- policy edits: evaluate the edited policies alone ----
    def apply_edit(self, full, edited, removed=()):
        """`apply` for the usual event, one policy edited, added or removed out of hundreds: only
        `edited`, a PolicySet of the edited and added policies alone (with the exceptions naming
        them), is evaluated, its columns are spliced into the kept matrix on the device and the
        columns of the `removed` policies (names) are dropped (Engine.splice_results). The
        background controller likewise keeps the stored results of unchanged policies and
        recomputes only the changed ones (controller.go:379-419); a rule's verdict depends on no
        other policy. Returns {row: verdict row under the new set}, the rows `apply(full,
        edited=names of edited)` would return: FAIL / ERROR / SKIP cells of `edited` always count.

        full: the complete new PolicySet, or a zero-argument callable returning it, called only when
        something needs the whole set (namespace_counts, cli_summary, reports, matrix, update,
        set_namespace_labels, compact(reflatten=True), which evaluate it first; a compaction by
        gather leaves it alone). Rules are paired by name, so the
        rules of `edited` must carry the names they have in `full`.

        keep="matrix" only: keep="fingerprints" raises ValueError, since a fingerprint cannot give
        back the old cells of the edited policy to take them out. KPE_E_STATE before the first
        `apply`. Check masks and traces of the unchanged policies are not kept: reports render them
        from a full evaluation, reports(rows, policies="edited") renders the edited policies'
        entries from this one. Costs a second matrix buffer per segment on the device."""
        if self.keep == "fingerprints":
            raise ValueError('apply_edit: keep="matrix" only (a fingerprint cannot give back the old cells)')
        if self._applied_v is None or self._policies is None:
            raise KpeError(5, "no apply yet")  # KPE_E_STATE
        eng = self.engine
        removed = list(removed)
        if edited.num_rules:  # nothing to evaluate when policies are only removed
            eng.evaluate_batch_async(edited, self._segs, masks=self._with_reports)
        self._edit, self._edit_ok = edited, True
        self._stale = True  # the segments' last evaluation is not of the applied set: _refresh evaluates it
        always = np.full(edited.num_rules, self.MESSAGE_CODES, dtype=np.uint8)
        out = {}
        for s, seg in enumerate(self._segs):
            total = eng.splice_results(edited, seg, removed, always)
            if not total:
                continue
            rows, vr, _ = eng.spliced_rows(seg, cap=total)
            if self._keyed:
                for k, l in self._map.translate(s, rows):
                    out[l] = vr[k].copy()
            else:
                out.update((int(i), vr[k].copy()) for k, i in enumerate(rows))
        self._applied = full
        self._policies = full
        self.last_stats = {"rows": self._map.n_live if self._keyed else self.corpus.n, "changed": len(out),
                           "segments": len(self._segs), "partial": True, "columns": edited.num_rules}
        return out

    # ---- resource churn (keyed=True) ----
    def _need_keyed(self):
        if not self._keyed:
            raise KpeError(5, "ResidentScanner(keyed=True) follows resource churn")  # KPE_E_STATE

    def _apply_segments(self, policies, always, msg):
        """`apply` over the segments: one batch evaluation, the per-segment changed rows translated
        to logical rows (rows of retired physical rows dropped). always: keep="matrix"; msg: the
        msg_salts of keep="fingerprints"."""
        eng, m = self.engine, self._map
        eng.evaluate_batch_async(policies, self._segs, masks=self._with_reports)
        self._applied = policies
        self._stale, self._edit, self._unevaluated = False, None, False
        out = {}
        for s, seg in enumerate(self._segs):
            if msg is not None:
                if eng.kept_fingerprints(seg, 0, 0) is None:  # against "no report": every row with a response
                    eng.load_fingerprints(seg, np.zeros(seg.n, dtype=np.uint64))
                rows, vr, _, _ = eng.changed_rows_fp(policies, seg, msg_salts=msg, msg_codes=self.MESSAGE_CODES)
                eng.keep_fingerprints(policies, seg, msg_salts=msg, msg_codes=self.MESSAGE_CODES)
            elif self._policies is None:  # nothing to compare with: the whole matrix, once
                v, _, _ = eng.fetch(policies, seg)
                rows = np.flatnonzero((v != 0).any(axis=1))
                vr = v[rows]
            else:
                rows, vr, _ = eng.changed_rows(policies, seg, always=always)
            for k, l in m.translate(s, rows):
                out[l] = vr[k].copy()
            if msg is None:
                eng.keep_results(policies, seg)
        if msg is None:
            self._policies = policies
        self.last_stats = {"rows": m.n_live, "changed": len(out), "segments": len(self._segs)}
        return out

    def _keep(self, seg):
        """Keep the last evaluation of the applied PolicySet on seg, as `apply` does."""
        if self.keep == "fingerprints":
            self.engine.keep_fingerprints(self._applied, seg, msg_salts=self._msg, msg_codes=self.MESSAGE_CODES)
        else:
            self.engine.keep_results(self._applied, seg)

    def update(self, upserts: bytes = b"", deletes=()):
        """Resource events between two policy changes (background/controller.go:247-297,
        needsReconcile): `upserts` is NDJSON of created or changed resources, `deletes` keys (as
        `_key` makes them) or logical rows. Returns {logical row: verdict row, or None for a deleted
        resource} of exactly the rows whose report changes under the last applied PolicySet.

        An offered resource whose hash equals the stored one is dropped before flattening
        (last_stats["skipped"]). The others are flattened into a delta segment, a corpus of its
        own, evaluated with the last applied PolicySet; a replaced resource is compared on the
        device with the kept result of the segment that held it (Engine.changed_pairs, or
        changed_pairs_fp with keep="fingerprints"), a new one is reported when it has any response.
        Then the delta segment's result is kept and the replaced and deleted rows are retired in
        their old segments. Logical rows are stable: a resource keeps its index for life, new ones
        are appended, a deleted one's is never reused. Before the first `apply` there is nothing
        to compare: the corpus is restructured and {} returned."""
        self._need_keyed()
        eng, m = self.engine, self._map
        lines = ndjson_rows(upserts)
        deletes = list(deletes)
        relabel, relabelled = {}, 0
        if self._ns_objects:
            # a deleted resource is known by its stored line (a UID key says nothing of its kind), or
            # by its key alone when the corpus never held it
            gone = [d if m.row_of(d) is None else self._lines[m.row_of(d)] for d in deletes]
            events = namespace_label_events(lines, [g for g in gone if g is not None])
            if events:  # before the delta segment is flattened: it takes the new table
                relabel = self.set_namespace_labels(events)
                relabelled = self.last_stats["relabelled"]
        self._edit_ok = False  # the segments change: the partial evaluation's entries are no longer offered
        offered =list(zip((_key(r, i) for i, r in enumerate(lines)), resource_hashes(b"\n".join(lines)))) if lines else []
        plan = m.plan(offered, deletes)
        items = plan["items"]
        out = {}
        fresh = {}  # row of the delta segment -> verdict row, of the new resources that have a response
        seg = None
        if items:
            seg = Corpus(b"\n".join(lines[i] for i, _ in items), self._nsl).upload(eng.device)
            if seg.n != len(items):
                raise KpeError(2, "update: one corpus row per offered resource")  # KPE_E_INVALID
        if self._applied is not None:
            if seg is not None:
                eng.evaluate_async(self._applied, seg, masks=self._with_reports)
                by_old = {}  # old segment -> [(row of seg, logical row, old row)]
                for j, (_, l) in enumerate(items):
                    if l is not None:
                        by_old.setdefault(m.loc[l][0], []).append((j, l, m.loc[l][1]))
                for s, trip in by_old.items():
                    pairs = np.array([(j, r) for j, _, r in trip], dtype=np.uint64)
                    if self.keep == "fingerprints":
                        idx, vr, _, _ = eng.changed_pairs_fp(self._applied, seg, self._segs[s], pairs, msg_salts=self._msg,
                                                             msg_codes=self.MESSAGE_CODES)
                    else:
                        idx, vr, _ = eng.changed_pairs(self._applied, seg, self._segs[s], pairs)
                    for k, i in enumerate(idx):
                        out[trip[int(i)][1]] = vr[k].copy()
                if any(l is None for _, l in items):  # the delta is small: its matrix, for the new resources
                    v, _, _ = eng.fetch(self._applied, seg)
                    fresh = {j: v[j].copy() for j, (_, l) in enumerate(items) if l is None and v[j].any()}
                self._keep(seg)
            for l in plan["deletes"]:
                out[l] = None
        new_seg, rows, retire = m.commit(plan)
        if seg is not None:
            self._segs.append(seg)
            assert new_seg == len(self._segs) - 1
            for j, l in enumerate(rows):
                if l == len(self._lines):
                    self._lines.append(None)
                self._lines[l] = lines[items[j][0]]
            for j, row in fresh.items():
                out[rows[j]] = row
        for l in plan["deletes"]:
            self._lines[l] = None
        for s, rr in retire.items():
            eng.retire_rows(self._segs[s], rr)
            self._stale = True
        self._updated = True
        if relabel:  # the rows the label events changed; a row in both is what the update made of it
            out = {**relabel, **out}
        self.last_stats = {"rows": m.n_live, "offered": len(lines), "skipped": plan["skipped"], "rescanned": len(items),
                           "deleted": len(plan["deletes"]), "changed": len(out), "segments": len(self._segs)}
        if self._ns_objects:
            self.last_stats["relabelled"] = relabelled
        if m.needs_compaction():
            self.compact()
            self.last_stats["segments"] = len(self._segs)
            self.last_stats["compacted"] = True
        return out

    def compact(self, reflatten=False):
        """One segment again: the live rows in logical order. The segments are flattened already,
        so the new one is gathered from their rows (Corpus.gather: no JSON is parsed), uploaded,
        and the kept matrix or fingerprints of those rows are carried over on the device
        (Engine.gather_results). Nothing is compiled or evaluated, no fingerprint crosses to the
        host and a lazy `full` of apply_edit stays unresolved; the readers that need an evaluation
        of the applied set (matrix, reports, namespace_counts, cli_summary) evaluate first, as
        they do after rows were retired. Nothing is reported as changed: it is the state the
        segments already held.

        reflatten=True, or merged dictionaries past a limit the rows were flattened under
        (KPE_E_LIMIT): the live NDJSON lines are flattened again instead, the last applied
        PolicySet is evaluated on the result and that is kept; with keep="fingerprints" the kept
        fingerprints are carried over through the host (Engine.load_fingerprints)."""
        self._need_keyed()
        eng, m = self.engine, self._map
        if not reflatten:
            live = m.live()
            pairs = np.array([m.loc[l] for l in live], dtype=np.uint64).reshape(-1, 2)
            try:
                seg = Corpus.gather(self._segs, pairs)
            except KpeError as e:
                if e.status != 4:  # KPE_E_LIMIT: flatten again
                    raise
                seg = None
            if seg is not None:
                seg.upload(eng.device)
                if self.keep == "fingerprints":
                    # loaded fingerprints and an update before the first apply: the delta segments keep
                    # nothing. Their rows stand against "no report" (0), as in _apply_segments, so that
                    # every segment keeps fingerprints and the loaded ones are carried.
                    has = [eng.kept_fingerprints(s, 0, 0) is not None for s in self._segs]
                    if any(has) and not all(has):
                        for s, h in zip(self._segs, has):
                            if not h:
                                eng.load_fingerprints(s, np.zeros(s.n, dtype=np.uint64))
                eng.gather_results(seg, self._segs, pairs)
                m.compact()
                self._segs = [seg]
                self.corpus = seg
                self._edit = None
                self._stale = self._unevaluated = self._applied_v is not None
                self._updated = True
                return
        fps = self._fps_by_row() if self.keep == "fingerprints" else None
        had_fps = fps is not None and eng.kept_fingerprints(self._segs[0], 0, 0) is not None
        live = m.compact()
        seg = Corpus(b"\n".join(self._lines[l] for l in live), self._nsl).upload(eng.device)
        if seg.n != len(live):
            raise KpeError(2, "compact: one corpus row per live resource")  # KPE_E_INVALID
        self._segs = [seg]
        self.corpus = seg
        self._stale, self._edit, self._unevaluated = False, None, False
        if self._applied is not None:
            eng.evaluate_async(self._applied, seg, masks=self._with_reports)
            if self.keep != "fingerprints":
                eng.keep_results(self._applied, seg)
        if had_fps:
            eng.load_fingerprints(seg, fps[np.array(live, dtype=np.int64)])
        self._updated = True

    def matrix(self):
        """The current verdict matrix by logical row under the last applied PolicySet (a deleted
        resource's row is all NA): (logical rows, R) uint8. Diagnostics and tests: it fetches every
        segment's matrix."""
        self._need_keyed()
        if self._applied_v is None:
            raise KpeError(5, "no apply yet")
        if self._edit is not None or self._unevaluated:  # the last evaluation is of the edited policies alone, or none
            self._refresh()
        out = np.zeros((self._map.n_logical, self._applied.num_rules), dtype=np.uint8)
        for s, seg in enumerate(self._segs):
            v, _, _ = self.engine.fetch(self._applied, seg)
            back = np.array(self._map.back[s], dtype=np.int64)
            out[back[back >= 0]] = v[back >= 0]
        return out
