"""Host-side mirror of the reference engine interface, backed by libkpe.

Reference surface mirrored here (names and meaning kept):
  engineapi.Engine.Validate(ctx, PolicyContext) EngineResponse   pkg/engine/api/engine.go:17-23
  engineapi.EngineResponse / PolicyResponse.Rules                pkg/engine/api/engineresponse.go:14-60
  engineapi.RuleResponse (name, type, status)                    pkg/engine/api/ruleresponse.go:25-60
  engineapi.RuleStatus pass/fail/warning/error/skip              pkg/engine/api/rulestatus.go:4-21
  engine.NewPolicyContext(..., Create, ...).WithNewResource(r).WithPolicy(p).WithNamespaceLabels(l)
                                                                 pkg/controllers/report/utils/scanner.go:99-110
Single-resource Validate() is served by the same batch kernels (a batch of one);
batch callers (`kyverno apply`'s resource loop, the background scanner) use
Engine.validate_batch()/evaluate(), which evaluate the whole resource x rule
matrix on the GPU in one pass.
"""
import ctypes
import enum
import json
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np

from ._lib import CliTotals, Counts, KernelStats, KpeError, check, load


class RuleStatus(str, enum.Enum):
    PASS = "pass"
    FAIL = "fail"
    WARN = "warning"
    ERROR = "error"
    SKIP = "skip"


# kpe_verdict cell codes -> RuleStatus (0 = no RuleResponse)
VERDICT = {1: RuleStatus.PASS, 2: RuleStatus.FAIL, 3: RuleStatus.WARN, 4: RuleStatus.ERROR, 5: RuleStatus.SKIP}
UNDECIDED = 7  # kpe_verdict KPE_UNDECIDED: a cell the device leaves to the reference engine


@dataclass
class RuleResponse:
    name: str
    status: RuleStatus
    rule_type: str = "Validation"
    pod_security_checks: List[str] = field(default_factory=list)  # failing PSA check IDs (PSS rules)


@dataclass
class EngineResponse:
    policy: str
    resource: Optional[dict]
    rules: List[RuleResponse]

    def is_successful(self):  # engineresponse.go IsSuccessful: no fail/error rule
        return not any(r.status in (RuleStatus.FAIL, RuleStatus.ERROR) for r in self.rules)


@dataclass
class PolicyContext:
    """engine.NewPolicyContext(..., kyvernov1.Create, ...) for background/CLI scans."""
    resource: dict
    policy: dict
    namespace_labels: Dict[str, str] = field(default_factory=dict)
    operation: str = "CREATE"

    def with_new_resource(self, r):
        self.resource = r
        return self

    def with_policy(self, p):
        self.policy = p
        return self

    def with_namespace_labels(self, l):
        self.namespace_labels = dict(l or {})
        return self


class Device:
    def __init__(self, ordinal: int = 0):
        L = load()
        h = ctypes.c_void_p()
        check(L.kpe_device_open(int(ordinal), ctypes.byref(h)))
        self.h, self.ordinal = h, ordinal

    def close(self):
        if self.h:
            load().kpe_device_close(self.h)
            self.h = None

    def sync(self):
        check(load().kpe_device_sync(self.h))

    def set_timing(self, on: bool):
        check(load().kpe_device_set_timing(self.h, 1 if on else 0))

    def kernel_stats(self, reset=False):
        st = KernelStats()
        check(load().kpe_device_kernel_stats(self.h, None, None, ctypes.byref(st), 1 if reset else 0))
        return st

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PolicySet:
    """Compiled policies (autogen applied once, autogen.ComputeRules)."""

    def __init__(self, policies, exceptions=None, background=False):
        """exceptions: PolicyException objects (kyverno.io/v2beta1) or their JSON; background:
        drop exceptions with spec.background false, as the background scanner does."""
        L = load()
        if isinstance(policies, (bytes, str)):
            raw = policies if isinstance(policies, bytes) else policies.encode()
            self.policies = None
        else:
            self.policies = list(policies) if isinstance(policies, (list, tuple)) else [policies]
            raw = json.dumps(self.policies).encode()
        if exceptions is None:
            xraw = b""
        elif isinstance(exceptions, (bytes, str)):
            xraw = exceptions if isinstance(exceptions, bytes) else exceptions.encode()
        else:
            xraw = json.dumps(list(exceptions) if isinstance(exceptions, (list, tuple)) else [exceptions]).encode()
        self.exceptions = exceptions
        h = ctypes.c_void_p()
        check(L.kpe_program_compile_ex(raw, len(raw), xraw or None, len(xraw), 1 if background else 0, ctypes.byref(h)))
        self.h = h
        n = L.kpe_program_num_rules(h)
        self.rule_names = [L.kpe_program_rule_name(h, i).decode() for i in range(n)]
        self.is_pss = [bool(L.kpe_program_rule_is_pss(h, i)) for i in range(n)]

    @property
    def num_rules(self):
        return len(self.rule_names)

    def __del__(self):
        try:
            if self.h:
                load().kpe_program_free(self.h)
                self.h = None
        except Exception:
            pass


class Corpus:
    """Flattened, string-interned resources (host columns, optionally on a device)."""

    DOCS = 1  # KPE_CORPUS_DOCS: keep document tapes (pattern / anyPattern rules)

    def __init__(self, resources, namespace_labels: Optional[Dict[str, Dict[str, str]]] = None, docs: bool = True):
        L = load()
        if isinstance(resources, (bytes, bytearray)):
            raw = bytes(resources)
        elif isinstance(resources, str):
            raw = resources.encode()
        else:
            raw = "\n".join(json.dumps(r, separators=(",", ":")) for r in resources).encode()
        if isinstance(namespace_labels, (bytes, bytearray)):
            nsl = bytes(namespace_labels)
        else:
            nsl = json.dumps(namespace_labels).encode() if namespace_labels else b""
        h = ctypes.c_void_p()
        check(L.kpe_corpus_flatten_ex(raw, len(raw), nsl if nsl else None, len(nsl), self.DOCS if docs else 0,
                                      ctypes.byref(h)))
        self.h = h
        self.n = int(L.kpe_corpus_num_resources(h))
        self.nbytes = int(L.kpe_corpus_bytes(h))
        self.device = None

    @staticmethod
    def _gather_args(srcs, pairs):
        srcs = list(srcs)
        p = np.ascontiguousarray(pairs, dtype=np.uint64).reshape(-1, 2)
        hs = (ctypes.c_void_p * max(len(srcs), 1))(*[s.h for s in srcs])
        return srcs, p, hs

    @classmethod
    def gather(cls, srcs: Sequence["Corpus"], pairs) -> "Corpus":
        """A corpus out of chosen rows of other corpora (kpe_corpus_gather): pairs is (k, 2) of
        (index into srcs, row), and row k of the result is that row. No JSON is read; every
        consumer behaves as on a corpus flattened from those rows' lines in that order under the
        sources' namespace label table. The result is not uploaded, has nothing retired and keeps
        nothing. KpeError 1 (KPE_E_INVALID) for a pair outside its source or naming a retired row
        and for sources that differ in documents or label tables; 4 (KPE_E_LIMIT) when the merged
        dictionaries cross a limit: flatten the lines again."""
        L = load()
        srcs, p, hs = cls._gather_args(srcs, pairs)
        h = ctypes.c_void_p()
        check(L.kpe_corpus_gather(hs if srcs else None, len(srcs), p.ctypes.data if p.size else None, len(p),
                                  ctypes.byref(h)))
        self = cls.__new__(cls)
        self.h = h
        self.n = int(L.kpe_corpus_num_resources(h))
        self.nbytes = int(L.kpe_corpus_bytes(h))
        self.device = None
        return self

    def row_digests(self) -> np.ndarray:
        """One uint64 per row that holds no id and no position (kpe_corpus_row_digests): equal for
        two rows flattened from the same line under the same label table, in whatever corpus."""
        out = np.zeros(self.n, dtype=np.uint64)
        check(load().kpe_corpus_row_digests(self.h, out.ctypes.data if self.n else None))
        return out

    def row_flags(self) -> np.ndarray:
        """Per-row flatten status (kpe_corpus_row_flags): KPE_ROW_DECODE_ERROR = 1,
        KPE_ROW_LIMIT = 2, KPE_ROW_NO_SPEC = 4."""
        out = np.zeros(self.n, dtype=np.uint32)
        check(load().kpe_corpus_row_flags(self.h, out.ctypes.data))
        return out

    def digest(self) -> int:
        """64-bit digest of the columnar encoding (kpe_corpus_digest)."""
        return int(load().kpe_corpus_digest(self.h))

    @property
    def namespaces(self) -> List[str]:
        """Names of the corpus's namespace groups (kpe_corpus_namespace), by group id. A resource's
        group is its metadata.namespace (GetNamespace()); "" is the group of cluster-scoped
        resources (a Namespace object included) and always exists."""
        L = load()
        return [L.kpe_corpus_namespace(self.h, g).decode(errors="surrogateescape")
                for g in range(int(L.kpe_corpus_num_namespaces(self.h)))]

    def row_namespaces(self) -> np.ndarray:
        """The namespace group of every row (kpe_corpus_row_namespaces): (n,) uint32."""
        out = np.zeros(self.n, dtype=np.uint32)
        check(load().kpe_corpus_row_namespaces(self.h, out.ctypes.data if self.n else None))
        return out

    def namespace_rows(self) -> np.ndarray:
        """Rows per namespace group (kpe_corpus_namespace_rows): (G,) uint64, summing to n."""
        out = np.zeros(int(load().kpe_corpus_num_namespaces(self.h)), dtype=np.uint64)
        check(load().kpe_corpus_namespace_rows(self.h, out.ctypes.data))
        return out

    def namespace_labels(self) -> Dict[str, Dict[str, str]]:
        """The namespace label table as it is now (kpe_corpus_namespace_labels), in table order:
        what the constructor was given, after every Engine.set_namespace_labels since."""
        L = load()
        n = int(L.kpe_corpus_namespace_labels(self.h, None, 0))
        if n < 0:
            check(-n)
        buf = ctypes.create_string_buffer(max(n, 1))
        L.kpe_corpus_namespace_labels(self.h, buf, n)
        return json.loads(buf.raw[:n].decode(errors="surrogateescape"))

    def set_namespace_labels(self, labels, replace=False, device: Optional[Device] = None) -> int:
        """Engine.set_namespace_labels on this corpus; device defaults to the one it is uploaded to
        (none for a corpus that is not uploaded: the table then changes on the host alone)."""
        js = bytes(labels) if isinstance(labels, (bytes, bytearray)) else (
            b"" if labels is None else json.dumps(labels).encode())
        dev = device if device is not None else self.device
        n = ctypes.c_uint64(0)
        check(load().kpe_corpus_set_namespace_labels(dev.h if dev is not None else None, self.h, js if js else None, len(js),
                                                     NSL_REPLACE if replace else 0, ctypes.byref(n)))
        if n.value:
            self.nbytes = int(load().kpe_corpus_bytes(self.h))
        return int(n.value)

    def upload(self, dev: Device):
        check(load().kpe_corpus_upload(dev.h, self.h))
        self.device = dev
        return self

    def psa_summary(self) -> np.ndarray:
        """The per-pod PSA summary built on the corpus's device (kpe_corpus_psa_summary):
        n x 2 uint32 (schema.h PS_*)."""
        if self.device is None:
            raise KpeError(5, "corpus not uploaded")  # KPE_E_STATE
        out = np.zeros((self.n, 2), dtype=np.uint32)
        check(load().kpe_corpus_psa_summary(self.device.h, self.h, out.ctypes.data))
        return out

    def __del__(self):
        try:
            if self.h:
                load().kpe_corpus_free(self.h)
                self.h = None
        except Exception:
            pass


# kpe_synth_mix (include/kpe_synth.h)
SYNTH_PODS, SYNTH_MIXED, SYNTH_EDGE, SYNTH_SELECTORS, SYNTH_FANOUT, SYNTH_C3 = range(6)


def packed_words(cells: int) -> int:
    """32-bit words of a 3-bit packed verdict matrix of `cells` cells (10 cells per word)."""
    return int(load().kpe_packed_words(cells))


def unpack_verdicts(packed: np.ndarray, n: int, r: int) -> np.ndarray:
    """Host expansion of kpe_pack_verdicts output into an n x r uint8 verdict matrix."""
    packed = np.ascontiguousarray(packed, dtype=np.uint32)
    if packed.size < packed_words(n * r):
        raise ValueError("packed buffer too small")
    out = np.empty((n, r), dtype=np.uint8)
    check(load().kpe_unpack_verdicts(packed.ctypes.data, n * r, out.ctypes.data if n * r else None))
    return out


def evaluate_sharded(engines: Sequence["Engine"], ps: "PolicySet", shards: Sequence["Corpus"]):
    """One logical corpus over several devices of this process (kpe_evaluate_sharded): the
    shards' verdict rows in order and the summed per-rule counts."""
    L = load()
    k = len(shards)
    if len(engines) != k or k == 0:
        raise ValueError("one engine (device) per shard")
    for e, c in zip(engines, shards):
        if c.device is not e.device:
            c.upload(e.device)
    R = ps.num_rules
    N = sum(c.n for c in shards)
    v = np.zeros((N, R), dtype=np.uint8)
    counts = (Counts * max(R, 1))()
    devs = (ctypes.c_void_p * k)(*[e.device.h for e in engines])
    cps = (ctypes.c_void_p * k)(*[c.h for c in shards])
    check(L.kpe_evaluate_sharded(devs, cps, k, ps.h, v.ctypes.data if N * R else None, counts))
    cnt = [{"na": c.na, "pass": c.pass_, "fail": c.fail, "warn": c.warn, "error": c.error, "skip": c.skip,
            "undecided": c.undecided} for c in counts[:R]]
    return v, cnt


def synth_resources(seed: int, n: int, mix: int = 0, first_index: int = 0) -> bytes:
    """NDJSON from the synthetic generator (include/kpe_synth.h)."""
    L = load()
    p = ctypes.c_void_p()
    ln = ctypes.c_size_t()
    if L.kpe_synth_resources(seed, first_index, n, mix, ctypes.byref(p), ctypes.byref(ln)) != 0:
        raise KpeError(-1, "synth failed")
    try:
        # string_at's size is a C int in Python 3.10: corpora past 2 GiB are copied by array
        return bytes((ctypes.c_char * ln.value).from_address(p.value)) if ln.value else b""
    finally:
        L.kpe_synth_free(p)


def synth_ns_labels(seed: int, n_namespaces: int, mix: int = 0) -> bytes:
    """Namespace label table JSON from the synthetic generator (include/kpe_synth.h)."""
    L = load()
    p = ctypes.c_void_p()
    ln = ctypes.c_size_t()
    if L.kpe_synth_ns_labels(seed, n_namespaces, mix, ctypes.byref(p), ctypes.byref(ln)) != 0:
        raise KpeError(-1, "synth failed")
    try:
        # string_at's size is a C int in Python 3.10: corpora past 2 GiB are copied by array
        return bytes((ctypes.c_char * ln.value).from_address(p.value)) if ln.value else b""
    finally:
        L.kpe_synth_free(p)


class CorpusBatch:
    """Corpus handles packed once for kpe_evaluate_batch_async (keeps the corpora alive)."""

    def __init__(self, corpora: Sequence[Corpus]):
        self.corpora = list(corpora)
        self.n = len(self.corpora)
        self.arr = (ctypes.c_void_p * max(self.n, 1))(*[c.h for c in self.corpora])


class Engine:
    """engineapi.Engine (validate path) on one MI355X."""

    def __init__(self, device: Optional[Device] = None, ordinal: int = 0):
        self.device = device or Device(ordinal)

    # ---- columnar batch API ----
    def evaluate(self, ps: PolicySet, corpus: Corpus, check_masks=False):
        """Verdict matrix (N x R uint8, kpe_verdict), optional PSS check masks, per-rule counts."""
        L = load()
        if corpus.device is not self.device:
            corpus.upload(self.device)
        N, R = corpus.n, ps.num_rules
        v = np.zeros((N, R), dtype=np.uint8)
        m = np.zeros((N, R), dtype=np.uint32) if check_masks else None
        counts = (Counts * max(R, 1))()
        check(L.kpe_evaluate(self.device.h, ps.h, corpus.h, v.ctypes.data if N * R else None,
                             m.ctypes.data if (m is not None and N * R) else None, counts))
        cnt = [{"na": c.na, "pass": c.pass_, "fail": c.fail, "warn": c.warn, "error": c.error, "skip": c.skip,
                "undecided": c.undecided} for c in counts[:R]]
        return v, m, cnt

    def fetch(self, ps: PolicySet, corpus: Corpus, check_masks=False):
        """(verdicts, masks or None, counts) of the last enqueued evaluation of ps on corpus
        (kpe_fetch): the read-back half of evaluate_async / evaluate_batch_async."""
        N, R = corpus.n, ps.num_rules
        v = np.zeros((N, R), dtype=np.uint8)
        m = np.zeros((N, R), dtype=np.uint32) if check_masks else None
        counts = (Counts * max(R, 1))()
        check(load().kpe_fetch(self.device.h, ps.h, corpus.h, v.ctypes.data if N * R else None,
                               m.ctypes.data if (m is not None and N * R) else None, counts))
        cnt = [{"na": c.na, "pass": c.pass_, "fail": c.fail, "warn": c.warn, "error": c.error, "skip": c.skip,
                "undecided": c.undecided} for c in counts[:R]]
        return v, m, cnt

    CVM_XMATCH = 1 << 31  # KPE_CVM_XMATCH: a flag of FAIL cells, not a versioned check

    def cv_masks(self, ps: PolicySet, corpus: Corpus, raw=False):
        """Failing versioned PSS checks (N x R uint32, bit v = kpe_pss_cv_check(v)) of the last
        evaluation with check_masks=True (kpe_fetch_cv_masks). Bit 31 (KPE_CVM_XMATCH: the
        cell's podSecurity PolicyException matched) is cleared unless raw=True; the report
        functions take the raw words."""
        m = np.zeros((corpus.n, ps.num_rules), dtype=np.uint32)
        if m.size:
            check(load().kpe_fetch_cv_masks(self.device.h, ps.h, corpus.h, m.ctypes.data))
        return m if raw else m & np.uint32(0x7FFFFFFF)

    def evaluate_async(self, ps: PolicySet, corpus: Corpus, masks=False, cold=False):
        """Enqueue one evaluation (results stay on the device). masks: also write the check masks;
        cold: re-run the per-corpus prologue (dictionary pass, prologue image)."""
        if not masks and not cold:
            check(load().kpe_evaluate_async(self.device.h, ps.h, corpus.h))
        else:
            check(load().kpe_evaluate_async_ex(self.device.h, ps.h, corpus.h, (1 if masks else 0) | (2 if cold else 0)))

    def batch(self, corpora: Sequence[Corpus]) -> "CorpusBatch":
        """A reusable list of corpora on this engine's device for evaluate_batch_async."""
        for c in corpora:
            if c.device is not self.device:
                raise KpeError(5, "corpus not uploaded to this engine's device")  # KPE_E_STATE
        return CorpusBatch(corpora)

    def evaluate_batch_async(self, ps: PolicySet, batch, masks=False, cold=False):
        """Enqueue one evaluation per corpus of `batch` (a CorpusBatch or a list), in order, with
        one call (kpe_evaluate_batch_async)."""
        b = batch if isinstance(batch, CorpusBatch) else self.batch(batch)
        check(load().kpe_evaluate_batch_async(self.device.h, ps.h, b.arr, b.n, (1 if masks else 0) | (2 if cold else 0)))

    # ---- verdict exchange (device-resident) ----
    def device_verdicts(self, ps: PolicySet, corpus: Corpus):
        """(device address, bytes) of the corpus's verdict matrix after an evaluation of ps."""
        ptr, nb = ctypes.c_void_p(), ctypes.c_uint64()
        check(load().kpe_device_verdicts(self.device.h, ps.h, corpus.h, ctypes.byref(ptr), ctypes.byref(nb)))
        return ptr.value, nb.value

    def pack_verdicts(self, ps: PolicySet, corpus: Corpus, dst_ptr: int, words: int):
        """3-bit packing of the verdict matrix into device memory at dst_ptr (kpe_pack_verdicts)."""
        check(load().kpe_pack_verdicts(self.device.h, ps.h, corpus.h, ctypes.c_void_p(dst_ptr), words))

    # ---- sparse result fetch (device-side selection and row summaries) ----
    def select_cells(self, ps: PolicySet, corpus: Corpus, sel, cap: Optional[int] = None, with_verdicts=True):
        """The selected cells of the last evaluation of ps on corpus (kpe_select_cells), in
        ascending cell index: (cells uint64 = row * R + column, their verdicts uint8, total).
        sel: a mask of kpe_verdict bits (SEL(v), SEL_RESPONSES) for every rule, or one per rule.
        cap: at most that many cells come back (total still counts all of them); None: a count
        call, then a call of exactly that size. cells is the list pattern_traces takes."""
        L = load()
        R = ps.num_rules
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(sel, dtype=np.uint8), (R,)) if np.ndim(sel) == 0
                                 else np.asarray(sel, dtype=np.uint8))
        if s.shape != (R,):
            raise ValueError("sel: one mask, or one per rule")
        sbuf = s if R else np.zeros(1, dtype=np.uint8)

        def call(cells, verd, n):
            t = L.kpe_select_cells(self.device.h, ps.h, corpus.h, sbuf.ctypes.data, cells.ctypes.data if n else None,
                                   verd.ctypes.data if (verd is not None and n) else None, n)
            if t < 0:
                check(-t)
            return int(t)

        n = call(None, None, 0) if cap is None else min(int(cap), corpus.n * R)  # never more than every cell
        cells = np.zeros(n, dtype=np.uint64)
        verd = np.zeros(n, dtype=np.uint8) if with_verdicts else None
        total = call(cells, verd, n) if (n or cap is not None) else 0
        k = min(total, n)
        return cells[:k], (verd[:k] if with_verdicts else np.zeros(0, dtype=np.uint8)), total

    def row_summaries(self, ps: PolicySet, corpus: Corpus, row0: int = 0, nrows: Optional[int] = None) -> np.ndarray:
        """The report `summary` counters of rows [row0, row0 + nrows) of the last evaluation of ps
        on corpus, counted on the device (kpe_fetch_row_summaries): (nrows, 6) uint16, columns
        SUMMARY_FIELDS (pass, fail, warn, error, skip, undecided)."""
        n = corpus.n - row0 if nrows is None else nrows
        out = np.zeros((max(n, 0), 6), dtype=np.uint16)
        check(load().kpe_fetch_row_summaries(self.device.h, ps.h, corpus.h, row0, n, out.ctypes.data if n > 0 else None))
        return out

    def namespace_counts(self, ps: PolicySet, corpus: Corpus, g0: int = 0, ng: Optional[int] = None) -> np.ndarray:
        """Per-namespace rule counts of groups [g0, g0 + ng) of the last evaluation of ps on
        corpus, reduced on the device (kpe_fetch_namespace_counts): (ng, R, 6) uint32, last axis
        NS_COUNT_FIELDS (raw verdict codes: fail counts unscored fails too; NA is not counted)."""
        n = _ns_window(corpus, g0, ng)
        out = np.zeros((n, ps.num_rules, 6), dtype=np.uint32)
        check(load().kpe_fetch_namespace_counts(self.device.h, ps.h, corpus.h, g0, n, out.ctypes.data if n else None))
        return out

    # ---- result deltas (a kept matrix per corpus, the rows that changed against it) ----
    def keep_results(self, ps: PolicySet, corpus: Corpus):
        """Keep the verdict matrix of the last evaluation of ps on corpus on the device
        (kpe_results_keep: N x R bytes of HBM until drop_results or a re-upload), for changed_rows /
        delta_transitions after the next evaluation."""
        check(load().kpe_results_keep(self.device.h, ps.h, corpus.h))

    def drop_results(self, corpus: Corpus):
        check(load().kpe_results_drop(self.device.h, corpus.h))

    def kept_rule_names(self, corpus: Corpus) -> Optional[List[str]]:
        """The rule names of the kept result, or None when nothing is kept."""
        L = load()
        r = L.kpe_results_kept_rules(corpus.h)
        return None if r < 0 else [L.kpe_results_kept_rule_name(corpus.h, i).decode() for i in range(r)]

    def _delta_map(self, ps: PolicySet, column_map):
        if column_map is None:
            return None
        m = np.ascontiguousarray(column_map, dtype=np.int32)
        if m.shape != (ps.num_rules,):
            raise ValueError("column_map: one entry per rule of ps")
        return m if m.size else np.zeros(1, dtype=np.int32)

    def changed_rows(self, ps: PolicySet, corpus: Corpus, column_map=None, always=0, cap: Optional[int] = None,
                     with_verdicts=True):
        """The rows of the last evaluation of ps on corpus that differ from the kept result
        (kpe_changed_rows): (rows uint64 ascending, their verdict rows (k, R) uint8, total).
        column_map: the kept column of each rule of ps or -1 (None: by rule name); always: a mask of
        kpe_verdict bits (SEL(v)) per rule, or one for all: cells whose verdict is in it count as
        changed. cap: at most that many rows come back; None: a count call, then one of that size."""
        L = load()
        R = ps.num_rules
        mbuf = self._delta_map(ps, column_map)
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(always, dtype=np.uint8), (R,)) if np.ndim(always) == 0
                                 else np.asarray(always, dtype=np.uint8))
        if a.shape != (R,):
            raise ValueError("always: one mask, or one per rule")
        abuf = a if R else np.zeros(1, dtype=np.uint8)

        def call(rows, vr, n):
            t = L.kpe_changed_rows(self.device.h, ps.h, corpus.h, None if mbuf is None else mbuf.ctypes.data,
                                   abuf.ctypes.data, rows.ctypes.data if n else None,
                                   vr.ctypes.data if (vr is not None and n and R) else None, n)
            if t < 0:
                check(-t)
            return int(t)

        n = call(None, None, 0) if cap is None else min(int(cap), corpus.n)
        rows = np.zeros(n, dtype=np.uint64)
        vr = np.zeros((n, R), dtype=np.uint8) if with_verdicts else None
        total = call(rows, vr, n) if (n or cap is not None) else 0
        k = min(total, n)
        return rows[:k], (vr[:k] if with_verdicts else np.zeros((0, R), dtype=np.uint8)), total

    # ---- policy edits on a kept result (evaluate the edited policies alone, splice their columns in) ----
    @staticmethod
    def _names_arg(names):
        b = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
        return (ctypes.c_char_p * max(len(b), 1))(*b), len(b)

    def splice_plan(self, sub: PolicySet, corpus: Corpus, removed=()) -> np.ndarray:
        """The column plan kpe_results_splice would follow (kpe_splice_plan; host only): per column
        of the new kept matrix the kept column it copies, or -1 - s for column s of sub."""
        arr, k = self._names_arg(removed)
        L = load()
        rn = L.kpe_splice_plan(corpus.h, sub.h, arr, k, None, 0)
        if rn < 0:
            check(-rn)
        plan = np.zeros(max(rn, 1), dtype=np.int32)
        rn = L.kpe_splice_plan(corpus.h, sub.h, arr, k, plan.ctypes.data, rn)
        if rn < 0:
            check(-rn)
        return plan[:rn]

    def splice_results(self, sub: PolicySet, corpus: Corpus, removed=(), always=0) -> int:
        """After an evaluation of `sub` (the edited and added policies compiled alone) on a corpus
        with a kept result: splice its columns into the kept matrix, drop the columns of the
        `removed` policies (kpe_results_splice) and return the number of changed rows; the kept
        result and kept_rule_names are then the new PolicySet's. always: a mask of kpe_verdict
        bits (SEL(v)) per rule of sub, or one for all. Costs a second matrix buffer on the device."""
        R = sub.num_rules
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(always, dtype=np.uint8), (R,)) if np.ndim(always) == 0
                                 else np.asarray(always, dtype=np.uint8))
        if a.shape != (R,):
            raise ValueError("always: one mask, or one per rule of sub")
        abuf = a if R else np.zeros(1, dtype=np.uint8)
        arr, k = self._names_arg(removed)
        t = load().kpe_results_splice(self.device.h, sub.h, corpus.h, arr, k, abuf.ctypes.data)
        if t < 0:
            check(-t)
        return int(t)

    def spliced_rows(self, corpus: Corpus, with_verdicts=True, cap: Optional[int] = None):
        """The changed rows of the last splice_results on corpus (kpe_spliced_rows): (rows uint64
        ascending, their rows of the new kept matrix (k, R) uint8, total). cap: at most that many
        rows come back; None: a count call, then one of that size. Nothing is compared again."""
        L = load()
        R = max(L.kpe_results_kept_rules(corpus.h), 0)

        def call(rows, vr, n):
            t = L.kpe_spliced_rows(self.device.h, corpus.h, rows.ctypes.data if n else None,
                                   vr.ctypes.data if (vr is not None and n and R) else None, n)
            if t < 0:
                check(-t)
            return int(t)

        n = call(None, None, 0) if cap is None else min(int(cap), corpus.n)
        rows = np.zeros(n, dtype=np.uint64)
        vr = np.zeros((n, R), dtype=np.uint8) if with_verdicts else None
        total = call(rows, vr, n) if (n or cap is not None) else 0
        k = min(total, n)
        return rows[:k], (vr[:k] if with_verdicts else np.zeros((0, R), dtype=np.uint8)), total

    def kept_results(self, corpus: Corpus) -> Optional[np.ndarray]:
        """The kept matrix (N x kept R uint8), read back whole (kpe_results_kept_fetch): diagnostics
        and tests. None when nothing is kept."""
        L = load()
        R = L.kpe_results_kept_rules(corpus.h)
        if R < 0:
            return None
        out = np.zeros((corpus.n, R), dtype=np.uint8)
        check(L.kpe_results_kept_fetch(self.device.h, corpus.h, 0, corpus.n, out.ctypes.data if out.size else None))
        return out

    def delta_transitions(self, ps: PolicySet, corpus: Corpus, column_map=None) -> np.ndarray:
        """Per rule of ps the 8 x 8 table [kept code, new code] of the corpus's rows
        (kpe_delta_transitions): (R, 8, 8) uint64; the kept code is KPE_NA for an unmapped rule."""
        R = ps.num_rules
        mbuf = self._delta_map(ps, column_map)
        out = np.zeros((R, 8, 8), dtype=np.uint64)
        check(load().kpe_delta_transitions(self.device.h, ps.h, corpus.h, None if mbuf is None else mbuf.ctypes.data,
                                           out.ctypes.data if R else None))
        return out

    # ---- row fingerprints (8 bytes per row: kept, stored by the caller, compared on the device) ----
    def row_fingerprints(self, ps: PolicySet, corpus: Corpus, salts=None, msg_salts=None, msg_codes=None, masks=False,
                         row0: int = 0, nrows: Optional[int] = None) -> np.ndarray:
        """The fingerprints of rows [row0, row0 + nrows) of the last evaluation of ps on corpus
        (kpe_fetch_row_fingerprints): (nrows,) uint64. salts: one per rule (None: rule_salts(ps));
        msg_salts: the salts of the cells whose verdict is in msg_codes (None: salts; msg_codes None:
        MESSAGE_CODES); masks: FAIL cells' check mask words count (the evaluation wrote masks)."""
        n = corpus.n - row0 if nrows is None else nrows
        s, ms, mc = _fp_salts(ps.num_rules, salts, msg_salts, msg_codes)
        out = np.zeros(max(n, 0), dtype=np.uint64)
        check(load().kpe_fetch_row_fingerprints(self.device.h, ps.h, corpus.h, _ptr(s), _ptr(ms), mc,
                                                FP_MASKS if masks else 0, row0, n, out.ctypes.data if n > 0 else None))
        return out

    def keep_fingerprints(self, ps: PolicySet, corpus: Corpus, salts=None, msg_salts=None, msg_codes=None, masks=False):
        """Keep the fingerprints of the last evaluation of ps on corpus on the device
        (kpe_fingerprints_keep: 8 N bytes of HBM until drop_fingerprints or a re-upload), for
        changed_rows_fp after the next evaluation. Arguments as row_fingerprints."""
        s, ms, mc = _fp_salts(ps.num_rules, salts, msg_salts, msg_codes)
        check(load().kpe_fingerprints_keep(self.device.h, ps.h, corpus.h, _ptr(s), _ptr(ms), mc, FP_MASKS if masks else 0))

    def load_fingerprints(self, corpus: Corpus, fingerprints):
        """Restore stored fingerprints, one per row of corpus, as the kept ones (kpe_fingerprints_load)."""
        fp = np.ascontiguousarray(fingerprints, dtype=np.uint64)
        if fp.ndim != 1:
            raise ValueError("fingerprints: one uint64 per row")
        check(load().kpe_fingerprints_load(self.device.h, corpus.h, fp.ctypes.data if fp.size else None, fp.size))

    def kept_fingerprints(self, corpus: Corpus, row0: int = 0, nrows: Optional[int] = None) -> Optional[np.ndarray]:
        """The kept fingerprints of rows [row0, row0 + nrows) (kpe_fingerprints_fetch), or None when
        nothing is kept: what a caller stores with the reports."""
        L = load()
        if not L.kpe_fingerprints_kept(corpus.h):
            return None
        n = corpus.n - row0 if nrows is None else nrows
        out = np.zeros(max(n, 0), dtype=np.uint64)
        check(L.kpe_fingerprints_fetch(self.device.h, corpus.h, row0, n, out.ctypes.data if n > 0 else None))
        return out

    def drop_fingerprints(self, corpus: Corpus):
        check(load().kpe_fingerprints_drop(self.device.h, corpus.h))

    def gather_results(self, dst: Corpus, srcs: Sequence[Corpus], pairs, what: int = 0):
        """Carry kept results into a gathered corpus on the device (kpe_results_gather): dst
        (uploaded, one row per pair, as Corpus.gather(srcs, pairs) makes it) receives the kept
        matrix rows (GATHER_MATRIX) and / or kept fingerprints (GATHER_FINGERPRINTS) of the listed
        rows of srcs; what=0: whatever every listed source keeps. Nothing is evaluated and nothing
        crosses to the host."""
        srcs, p, hs = Corpus._gather_args(srcs, pairs)
        check(load().kpe_results_gather(self.device.h, dst.h, hs if srcs else None, len(srcs),
                                        p.ctypes.data if p.size else None, len(p), what))

    def changed_rows_fp(self, ps: PolicySet, corpus: Corpus, salts=None, msg_salts=None, msg_codes=None, masks=False,
                        cap: Optional[int] = None, with_verdicts=True):
        """The rows whose fingerprint under the last evaluation of ps on corpus differs from the
        kept one (kpe_changed_rows_fp): (rows uint64 ascending, their verdict rows (k, R) uint8,
        their new fingerprints (k,) uint64, total). The kept fingerprints stay as they are. cap: at
        most that many rows come back; None: a count call, then one of that size."""
        L = load()
        R = ps.num_rules
        s, ms, mc = _fp_salts(R, salts, msg_salts, msg_codes)
        fl = FP_MASKS if masks else 0

        def call(rows, vr, fps, n):
            t = L.kpe_changed_rows_fp(self.device.h, ps.h, corpus.h, _ptr(s), _ptr(ms), mc, fl,
                                      rows.ctypes.data if n else None,
                                      vr.ctypes.data if (vr is not None and n and R) else None,
                                      fps.ctypes.data if n else None, n)
            if t < 0:
                check(-t)
            return int(t)

        n = call(None, None, None, 0) if cap is None else min(int(cap), corpus.n)
        rows = np.zeros(n, dtype=np.uint64)
        fps = np.zeros(n, dtype=np.uint64)
        vr = np.zeros((n, R), dtype=np.uint8) if with_verdicts else None
        total = call(rows, vr, fps, n) if (n or cap is not None) else 0
        k = min(total, n)
        return rows[:k], (vr[:k] if with_verdicts else np.zeros((0, R), dtype=np.uint8)), fps[:k], total

    # ---- resource churn on a resident corpus (retired rows, delta corpora compared by pair) ----
    def retire_rows(self, corpus: Corpus, rows):
        """Retire rows of corpus (kpe_corpus_retire_rows): from the next evaluation on they give no
        response to any consumer. The set only grows and survives a re-upload; a corpus that is
        not uploaded records it on the host."""
        r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        check(load().kpe_corpus_retire_rows(self.device.h if corpus.device is not None else None, corpus.h,
                                            r.ctypes.data if r.size else None, r.size))

    def retired_rows(self, corpus: Corpus) -> np.ndarray:
        """The retired rows of corpus, ascending and unique (kpe_corpus_retired_rows): uint64."""
        L = load()
        n = int(L.kpe_corpus_retired_rows(corpus.h, None, 0))
        out = np.zeros(max(n, 0), dtype=np.uint64)
        if n > 0:
            L.kpe_corpus_retired_rows(corpus.h, out.ctypes.data, n)
        return out

    def set_namespace_labels(self, corpus: Corpus, labels, replace=False) -> int:
        """Change the namespace label table of a flattened (and possibly uploaded, evaluated)
        corpus in place (kpe_corpus_set_namespace_labels). labels: {namespace: {key: value}} or its
        JSON bytes; a patch by default ({namespace: None} removes an entry, namespaces not named
        keep theirs), with replace=True the whole table. Returns the number of namespaces whose
        entry changed; when it is not 0 the corpus has no last evaluation until the next one."""
        return corpus.set_namespace_labels(labels, replace, device=self.device if corpus.device is not None else None)

    @staticmethod
    def _pairs(pairs):
        p = np.ascontiguousarray(pairs, dtype=np.uint64).reshape(-1, 2)
        return p, (p if p.size else np.zeros((1, 2), dtype=np.uint64))

    def changed_pairs(self, ps: PolicySet, new: Corpus, old: Corpus, pairs, column_map=None, always=0,
                      cap: Optional[int] = None, with_verdicts=True):
        """For pairs (k, 2) of (row of new, row of old): the pairs whose row of the last evaluation
        of ps on `new` differs from the paired row of `old`'s kept result, by the rules of
        changed_rows (kpe_changed_pairs): (pair indices uint64 ascending, their new verdict rows
        (m, R) uint8, total). column_map, always, cap as in changed_rows."""
        L = load()
        R = ps.num_rules
        p, pbuf = self._pairs(pairs)
        mbuf = self._delta_map(ps, column_map)
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(always, dtype=np.uint8), (R,)) if np.ndim(always) == 0
                                 else np.asarray(always, dtype=np.uint8))
        if a.shape != (R,):
            raise ValueError("always: one mask, or one per rule")
        abuf = a if R else np.zeros(1, dtype=np.uint8)

        def call(idx, vr, n):
            t = L.kpe_changed_pairs(self.device.h, ps.h, new.h, old.h, pbuf.ctypes.data, len(p),
                                    None if mbuf is None else mbuf.ctypes.data, abuf.ctypes.data,
                                    idx.ctypes.data if n else None,
                                    vr.ctypes.data if (vr is not None and n and R) else None, n)
            if t < 0:
                check(-t)
            return int(t)

        n = call(None, None, 0) if cap is None else min(int(cap), len(p))
        idx = np.zeros(n, dtype=np.uint64)
        vr = np.zeros((n, R), dtype=np.uint8) if with_verdicts else None
        total = call(idx, vr, n) if (n or cap is not None) else 0
        k = min(total, n)
        return idx[:k], (vr[:k] if with_verdicts else np.zeros((0, R), dtype=np.uint8)), total

    def changed_pairs_fp(self, ps: PolicySet, new: Corpus, old: Corpus, pairs, salts=None, msg_salts=None,
                         msg_codes=None, masks=False, cap: Optional[int] = None, with_verdicts=True):
        """The fingerprint form (kpe_changed_pairs_fp): the pairs whose new row's fingerprint differs
        from `old`'s kept fingerprint of the paired row: (pair indices, their new verdict rows, their
        new fingerprints, total). Arguments as changed_rows_fp."""
        L = load()
        R = ps.num_rules
        p, pbuf = self._pairs(pairs)
        s, ms, mc = _fp_salts(R, salts, msg_salts, msg_codes)
        fl = FP_MASKS if masks else 0

        def call(idx, vr, fps, n):
            t = L.kpe_changed_pairs_fp(self.device.h, ps.h, new.h, old.h, pbuf.ctypes.data, len(p), _ptr(s), _ptr(ms),
                                       mc, fl, idx.ctypes.data if n else None,
                                       vr.ctypes.data if (vr is not None and n and R) else None,
                                       fps.ctypes.data if n else None, n)
            if t < 0:
                check(-t)
            return int(t)

        n = call(None, None, None, 0) if cap is None else min(int(cap), len(p))
        idx = np.zeros(n, dtype=np.uint64)
        fps = np.zeros(n, dtype=np.uint64)
        vr = np.zeros((n, R), dtype=np.uint8) if with_verdicts else None
        total = call(idx, vr, fps, n) if (n or cap is not None) else 0
        k = min(total, n)
        return idx[:k], (vr[:k] if with_verdicts else np.zeros((0, R), dtype=np.uint8)), fps[:k], total

    def pattern_traces(self, ps: PolicySet, corpus: Corpus, cells) -> np.ndarray:
        """Failing-path records of pattern cells (kpe_pattern_traces) after an evaluation of ps on
        corpus: cells = flat indices row * R + column; returns (len(cells), KPE_TRACE_ROOTS,
        KPE_TRACE_WORDS) uint32."""
        c = np.ascontiguousarray(cells, dtype=np.uint64)
        out = np.zeros((c.size, TRACE_ROOTS, TRACE_WORDS), dtype=np.uint32)
        if c.size:
            check(load().kpe_pattern_traces(self.device.h, ps.h, corpus.h, c.ctypes.data, c.size, out.ctypes.data))
        return out

    def row_traces(self, ps: PolicySet, corpus: Corpus, row: int) -> np.ndarray:
        """Trace records of every cell of one row (the layout report_results(traces=) takes)."""
        R = ps.num_rules
        return self.pattern_traces(ps, corpus, np.arange(row * R, row * R + R, dtype=np.uint64))

    def cond_traces(self, ps: PolicySet, corpus: Corpus, row0: int = 0, nrows: Optional[int] = None,
                    ex: bool = False) -> np.ndarray:
        """Condition traces (kpe_fetch_cond_traces) of rows [row0, row0 + nrows) after an evaluation
        of ps on corpus: (nrows, R) uint32, the layout report_results(cond_traces=) takes per row.
        ex: kpe_fetch_cond_traces_ex, (nrows, R, KPE_CTRACE_WORDS) with the foreach and error
        records (foreach messages, RuleError texts)."""
        n = corpus.n - row0 if nrows is None else nrows
        out = np.zeros((n, ps.num_rules, CTRACE_WORDS) if ex else (n, ps.num_rules), dtype=np.uint32)
        if n:
            f = load().kpe_fetch_cond_traces_ex if ex else load().kpe_fetch_cond_traces
            check(f(self.device.h, ps.h, corpus.h, row0, n, out.ctypes.data))
        return out

    # ---- reports for a row list (the sparse detail of the listed rows, then one bulk render) ----
    def fetch_report_rows(self, ps: PolicySet, corpus: Corpus, rows, masks=True, cond=True, patterns=True,
                          caps=None) -> dict:
        """What the reports of `rows` (row ids of corpus, any order, duplicates allowed) need beyond
        their verdicts, gathered on the device after an evaluation of ps on corpus
        (kpe_fetch_report_rows): a dict of verdict_rows (k, R) uint8 and three sparse lists over
        compact cells (position in rows * R + column): mask_cells / mask_words (the raw cv mask
        words, KPE_CVM_XMATCH included), cond_cells / cond_words (m, KPE_CTRACE_WORDS),
        pattern_cells / pattern_traces (m, KPE_TRACE_ROOTS, KPE_TRACE_WORDS), and the device totals
        mask_total, cond_total, pattern_total. masks needs an evaluation with masks. caps: at most
        that many entries per list (mask, cond, pattern); None: a count call, then an exact one."""
        r = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        rbuf = r if r.size else np.zeros(1, dtype=np.uint64)
        flags = _rr_flags(masks, cond, patterns)

        def call(io):
            check(load().kpe_fetch_report_rows(self.device.h, ps.h, corpus.h, rbuf.ctypes.data, r.size, flags,
                                               ctypes.byref(io)))

        return _rr_two_calls(call, r.size, ps.num_rules, caps, records=True)

    def report_rows(self, ps: PolicySet, corpus: Corpus, rows, resources=None, masks=True, cond=True,
                    patterns=True) -> List[List[dict]]:
        """The PolicyReport results of each listed row of the last evaluation of ps on corpus, as
        report_results gives them with the row's traces, condition traces and raw mask words: one
        fetch_report_rows (a count call and an exact call) and one render_report_rows. resources: a
        list aligned with rows of dicts or JSON bytes (None entries, or None: no messages)."""
        sp = self.fetch_report_rows(ps, corpus, rows, masks=masks, cond=cond, patterns=patterns)
        return render_report_rows(ps, sp, resources=resources, corpus=corpus)

    # ---- reference-shaped API ----
    def validate_batch(self, policies: Sequence[dict], resources: Sequence[dict],
                       namespace_labels: Optional[Dict[str, Dict[str, str]]] = None) -> List[List[EngineResponse]]:
        """EngineResponse per (resource, policy), rules in ComputeRules order, NA cells omitted."""
        ps = PolicySet(list(policies))
        corpus = Corpus(resources, namespace_labels)
        v, m, _ = self.evaluate(ps, corpus, check_masks=True)
        L = load()
        check_ids = [L.kpe_pss_check_id(k).decode() for k in range(17)]
        # policy boundaries by "<policy>/<rule>" prefix, in compile order
        spans, start = [], 0
        for p in policies:
            cnt = 0
            for x in ps.rule_names[start:]:
                if x.split("/", 1)[0] != p["metadata"]["name"]:
                    break
                cnt += 1
            spans.append((start, start + cnt))
            start += cnt
        out = []
        for i, res in enumerate(resources):
            row = []
            for (a, b), p in zip(spans, policies):
                rules = []
                for r in range(a, b):
                    cell = int(v[i, r])
                    if cell == 0:
                        continue
                    if cell == UNDECIDED:
                        raise KpeError(-1, f"cell ({i}, {ps.rule_names[r]}) is beyond the device's documented "
                                           "limits (KPE_UNDECIDED): evaluate it with the reference engine")
                    checks = [check_ids[k] for k in range(17) if (int(m[i, r]) >> k) & 1] if ps.is_pss[r] else []
                    rules.append(RuleResponse(ps.rule_names[r].split("/", 1)[1], VERDICT[cell],
                                              pod_security_checks=checks))
                row.append(EngineResponse(p["metadata"]["name"], res, rules))
            out.append(row)
        return out

    def validate(self, policy_context: PolicyContext) -> EngineResponse:
        """engineapi.Engine.Validate for one PolicyContext (a batch of one)."""
        nsl = None
        ns = (policy_context.resource.get("metadata") or {}).get("namespace")
        if ns and policy_context.namespace_labels:
            nsl = {ns: policy_context.namespace_labels}
        return self.validate_batch([policy_context.policy], [policy_context.resource], nsl)[0][0]


TRACE_WORDS, TRACE_ROOTS = 16, 4  # include/kpe.h KPE_TRACE_WORDS / KPE_TRACE_ROOTS
CTRACE_WORDS = 4  # include/kpe.h KPE_CTRACE_WORDS (kpe_fetch_cond_traces_ex)


class ReportArgs(ctypes.Structure):
    """include/kpe.h kpe_report_args"""
    _fields_ = [("prog", ctypes.c_void_p), ("corpus", ctypes.c_void_p), ("verdict_row", ctypes.c_void_p),
                ("cv_mask_row", ctypes.c_void_p), ("pattern_traces", ctypes.c_void_p),
                ("cond_traces", ctypes.c_void_p), ("resource_json", ctypes.c_char_p),
                ("resource_len", ctypes.c_size_t), ("cond_traces_ex", ctypes.c_void_p)]


def report_results(ps: PolicySet, verdict_row, cv_mask_row=None, resource=None, traces=None,
                   corpus: Optional[Corpus] = None, cond_traces=None) -> List[dict]:
    """EngineResponseToReportResults (pkg/utils/report/results.go:89-156) for one resource row,
    through kpe_report_results, or kpe_report_results_msg when the resource (a dict or its JSON
    bytes) is given: then results carry the RuleResponse message (podSecurity pass / fail,
    validate.pattern pass; no timestamp). With traces (Engine.row_traces of the row) and the
    corpus, kpe_report_results_msg_tr adds the pattern / anyPattern failure and anyPattern pass
    messages; with cond_traces (a row of Engine.cond_traces), kpe_report_results_ex adds the
    condition messages (preconditions skips, deny fails with condition messages)."""
    L = load()
    v = np.ascontiguousarray(verdict_row, dtype=np.uint8)
    m = None if cv_mask_row is None else np.ascontiguousarray(cv_mask_row, dtype=np.uint32)
    if v.size != ps.num_rules or (m is not None and m.size != ps.num_rules):
        raise ValueError("row length != number of rules")
    raw = None
    if resource is not None:
        raw = resource if isinstance(resource, (bytes, bytearray)) else json.dumps(resource).encode()
    cap = 4096
    while True:
        buf = ctypes.create_string_buffer(cap)
        mp = None if m is None else m.ctypes.data
        if raw is None:
            n = L.kpe_report_results(ps.h, v.ctypes.data, mp, buf, cap)
        elif cond_traces is not None:
            ct = np.ascontiguousarray(cond_traces, dtype=np.uint32)
            ex = ct.ndim == 2  # a row of Engine.cond_traces(ex=True): KPE_CTRACE_WORDS per rule
            if ct.size != ps.num_rules * (CTRACE_WORDS if ex else 1):
                raise ValueError("cond_traces: one word (or KPE_CTRACE_WORDS words) per rule of the row")
            t = None
            if traces is not None:
                t = np.ascontiguousarray(traces, dtype=np.uint32)
                if t.size != ps.num_rules * TRACE_ROOTS * TRACE_WORDS:
                    raise ValueError("traces: one record per rule of the row")
            a = ReportArgs(ps.h, corpus.h if corpus is not None else None, v.ctypes.data, mp,
                           None if t is None else t.ctypes.data, None if ex else ct.ctypes.data, raw, len(raw),
                           ct.ctypes.data if ex else None)
            n = L.kpe_report_results_ex(ctypes.byref(a), buf, cap)
        elif traces is not None:
            t = np.ascontiguousarray(traces, dtype=np.uint32)
            if t.size != ps.num_rules * TRACE_ROOTS * TRACE_WORDS:
                raise ValueError("traces: one record per rule of the row")
            n = L.kpe_report_results_msg_tr(ps.h, corpus.h if corpus is not None else None, v.ctypes.data, mp,
                                            t.ctypes.data, raw, len(raw), buf, cap)
        else:
            n = L.kpe_report_results_msg(ps.h, v.ctypes.data, mp, raw, len(raw), buf, cap)
        if n < 0:
            check(-n)
        if n < cap:
            return json.loads(buf.value.decode())
        cap = n + 1


RR_MASKS, RR_COND, RR_PATTERNS = 1, 2, 4  # include/kpe.h KPE_RR_*


class ReportRows(ctypes.Structure):
    """include/kpe.h kpe_report_rows"""
    _fields_ = [("verdict_rows", ctypes.c_void_p),
                ("mask_cells", ctypes.c_void_p), ("mask_words", ctypes.c_void_p), ("mask_cap", ctypes.c_uint64),
                ("cond_cells", ctypes.c_void_p), ("cond_words", ctypes.c_void_p), ("cond_cap", ctypes.c_uint64),
                ("pattern_cells", ctypes.c_void_p), ("pattern_traces", ctypes.c_void_p),
                ("pattern_cap", ctypes.c_uint64),
                ("mask_total", ctypes.c_uint64), ("cond_total", ctypes.c_uint64), ("pattern_total", ctypes.c_uint64)]


def _rr_flags(masks, cond, patterns) -> int:
    return (RR_MASKS if masks else 0) | (RR_COND if cond else 0) | (RR_PATTERNS if patterns else 0)


def _rr_two_calls(call, nrows: int, R: int, caps, records: bool) -> dict:
    """call(io) fills a kpe_report_rows; caps None: count first, then exactly that much."""
    if caps is None:
        io = ReportRows()
        call(io)
        caps = (io.mask_total, io.cond_total, io.pattern_total)
    cm, cc, cp = (int(x) for x in caps)
    v = np.zeros((nrows, R), dtype=np.uint8)
    a = {"mask_cells": np.zeros(cm, dtype=np.uint64), "mask_words": np.zeros(cm, dtype=np.uint32),
         "cond_cells": np.zeros(cc, dtype=np.uint64), "cond_words": np.zeros((cc, CTRACE_WORDS), dtype=np.uint32),
         "pattern_cells": np.zeros(cp, dtype=np.uint64),
         "pattern_traces": np.zeros((cp if records else 0, TRACE_ROOTS, TRACE_WORDS), dtype=np.uint32)}

    def p(name, n):
        return a[name].ctypes.data if n else None

    io = ReportRows(v.ctypes.data if (records and v.size) else None,
                    p("mask_cells", cm), p("mask_words", cm), cm, p("cond_cells", cc), p("cond_words", cc), cc,
                    p("pattern_cells", cp), p("pattern_traces", cp if records else 0), cp, 0, 0, 0)
    call(io)
    km, kc, kp = min(io.mask_total, cm), min(io.cond_total, cc), min(io.pattern_total, cp)
    out = {"verdict_rows": v, "mask_cells": a["mask_cells"][:km], "mask_words": a["mask_words"][:km],
           "cond_cells": a["cond_cells"][:kc], "cond_words": a["cond_words"][:kc],
           "pattern_cells": a["pattern_cells"][:kp], "pattern_traces": a["pattern_traces"][:kp if records else 0],
           "mask_total": int(io.mask_total), "cond_total": int(io.cond_total), "pattern_total": int(io.pattern_total)}
    return out


def report_detail_need(ps: PolicySet):
    """Which cells' report entries need which detail (kpe_report_detail_need): three (R,) uint8 arrays
    of SEL(v) bits per rule, (mask_sel, cond_sel, pattern_sel)."""
    R = ps.num_rules
    t = [np.zeros(max(R, 1), dtype=np.uint8) for _ in range(3)]
    check(load().kpe_report_detail_need(ps.h, t[0].ctypes.data, t[1].ctypes.data, t[2].ctypes.data))
    return tuple(x[:R] for x in t)


def report_cells(ps: PolicySet, verdict_rows, cv_mask_rows=None, cond_ex_rows=None, masks=True, cond=True, patterns=True,
                 caps=None) -> dict:
    """Engine.fetch_report_rows' selection over dense rows the caller holds (kpe_report_cells_host,
    the plain double loop; no device call): verdict_rows (k, R), cv_mask_rows (k, R) raw mask words,
    cond_ex_rows (k, R, KPE_CTRACE_WORDS). The same dict; pattern_traces is empty (there are no
    records without a device) and verdict_rows is the input. A kind without its input is not
    selected."""
    R = ps.num_rules
    v = np.ascontiguousarray(verdict_rows, dtype=np.uint8).reshape(-1, R) if R else np.zeros((0, 0), dtype=np.uint8)
    k = v.shape[0]
    m = None if cv_mask_rows is None else np.ascontiguousarray(cv_mask_rows, dtype=np.uint32).reshape(k, R)
    cx = None if cond_ex_rows is None else np.ascontiguousarray(cond_ex_rows, dtype=np.uint32).reshape(k, R, CTRACE_WORDS)
    flags = _rr_flags(masks and m is not None, cond and cx is not None, patterns)

    def call(io):
        check(load().kpe_report_cells_host(ps.h, k, v.ctypes.data if v.size else None, _ptr(m) if v.size else None,
                                           _ptr(cx) if v.size else None, flags, ctypes.byref(io)))

    out = _rr_two_calls(call, k, R, caps, records=False)
    out["verdict_rows"] = v
    return out


def render_report_rows(ps: PolicySet, sparse: dict, resources=None, corpus: Optional[Corpus] = None, raw=False):
    """The PolicyReport results of every row of a fetch_report_rows / report_cells dict in one
    multi-threaded call (kpe_report_results_rows): a list of result lists, one per row, each what
    report_results gives for the row's dense inputs. resources: aligned with the rows, dicts or JSON
    bytes (None entries, or None: no messages); corpus: for pattern and foreach messages. raw: the
    rows' JSON bytes instead of parsed lists."""
    R = ps.num_rules
    v = np.ascontiguousarray(sparse["verdict_rows"], dtype=np.uint8).reshape(-1, R) if R else np.zeros((0, 0), np.uint8)
    k = v.shape[0]
    arr = {n: np.ascontiguousarray(sparse[n], dtype=dt) for n, dt in
           (("mask_cells", np.uint64), ("mask_words", np.uint32), ("cond_cells", np.uint64), ("cond_words", np.uint32),
            ("pattern_cells", np.uint64), ("pattern_traces", np.uint32))}
    km, kc = arr["mask_cells"].size, arr["cond_cells"].size
    kp = min(arr["pattern_cells"].size, arr["pattern_traces"].size // (TRACE_ROOTS * TRACE_WORDS))

    def p(name, n):
        return arr[name].ctypes.data if n else None

    io = ReportRows(v.ctypes.data if v.size else None, p("mask_cells", km), p("mask_words", km), km,
                    p("cond_cells", kc), p("cond_words", kc), kc, p("pattern_cells", kp), p("pattern_traces", kp), kp,
                    km, kc, kp)
    res_p = lens = None
    keep = []
    if resources is not None:
        if len(resources) != k:
            raise ValueError("resources: one entry (or None) per row")
        keep = [None if r is None else (bytes(r) if isinstance(r, (bytes, bytearray)) else json.dumps(r).encode())
                for r in resources]
        res_p = (ctypes.c_char_p * max(k, 1))(*keep)
        lens = (ctypes.c_size_t * max(k, 1))(*[0 if r is None else len(r) for r in keep])
    offs = np.zeros(k + 1, dtype=np.uint64)
    cap = 1 << 16
    while True:
        buf = ctypes.create_string_buffer(cap)
        n = load().kpe_report_results_rows(ps.h, corpus.h if corpus is not None else None, k, ctypes.byref(io), res_p,
                                           lens, buf, cap, offs.ctypes.data)
        if n < 0:
            check(-n)
        if n < cap:
            break
        cap = n + 1
    data = buf.raw[:n]
    parts = [data[int(offs[i]):int(offs[i + 1])] for i in range(k)]
    return parts if raw else [json.loads(x.decode()) for x in parts]


SEL_RESPONSES = 0xFE  # include/kpe.h KPE_SEL_RESPONSES: every verdict code but KPE_NA
SUMMARY_FIELDS = ("pass", "fail", "warn", "error", "skip", "undecided")  # kpe_row_summary, in order


def SEL(v: int) -> int:
    """include/kpe.h KPE_SEL(v): the selection mask bit of verdict code v."""
    return 1 << int(v)


def row_summaries(ps: PolicySet, verdicts) -> np.ndarray:
    """CalculateSummary (pkg/utils/report/results.go:39-55) of each row of an (n, R) verdict
    matrix the caller holds, through kpe_row_summaries_host (no device call): (n, 6) uint16,
    columns SUMMARY_FIELDS. An unscored policy's fails count as warn; `undecided` counts the
    row's KPE_UNDECIDED cells."""
    v = np.ascontiguousarray(verdicts, dtype=np.uint8)
    R = ps.num_rules
    if v.ndim == 1:
        v = v.reshape(1, -1)
    if v.ndim != 2 or v.shape[1] != R:
        raise ValueError("verdicts: rows of one cell per rule")
    out = np.zeros((v.shape[0], 6), dtype=np.uint16)
    check(load().kpe_row_summaries_host(ps.h, v.ctypes.data if v.size else None, v.shape[0] if R else 0,
                                        out.ctypes.data if v.shape[0] else None))
    return out


def column_map(old_names: Sequence[str], new_names: Sequence[str]) -> np.ndarray:
    """The map kpe_delta_column_map builds, from two lists of "<policy>/<rule>" names: for each
    new rule the index of the old rule of the same name, or -1 (int32). A name that occurs twice
    on either side is KPE_E_INVALID, as there."""
    old = {}
    for i, nm in enumerate(old_names):
        if nm in old:
            raise KpeError(1, f"kept rule name occurs twice: {nm}")
        old[nm] = i
    if len(set(new_names)) != len(new_names):
        raise KpeError(1, "rule name occurs twice")
    return np.array([old.get(nm, -1) for nm in new_names], dtype=np.int32)


def _delta_args(Rn: int, cmap, always):
    m = np.ascontiguousarray(cmap, dtype=np.int32)
    if m.shape != (Rn,):
        raise ValueError("column_map: one entry per new rule")
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(always, dtype=np.uint8), (Rn,)) if np.ndim(always) == 0
                             else np.asarray(always, dtype=np.uint8))
    if a.shape != (Rn,):
        raise ValueError("always: one mask, or one per new rule")
    # a valid address for Rn == 0
    return (m if Rn else np.zeros(1, dtype=np.int32)), (a if Rn else np.zeros(1, dtype=np.uint8))


def _delta_matrices(old, new):
    o, v = np.ascontiguousarray(old, dtype=np.uint8), np.ascontiguousarray(new, dtype=np.uint8)
    if o.ndim != 2 or v.ndim != 2 or o.shape[0] != v.shape[0]:
        raise ValueError("old, new: verdict matrices of the same rows")
    return o, v


def changed_rows(old, new, column_map, always=0, cap: Optional[int] = None, with_verdicts=True):
    """The rows of `new` (n, Rn) that differ from `old` (n, Ro) under column_map (kpe_changed_rows'
    rule, through kpe_changed_rows_host; no device call): (rows uint64 ascending, their rows of
    `new` (k, Rn) uint8, total). always: a mask of kpe_verdict bits (SEL(v)) per new rule, or one
    for all; cap: at most that many rows come back."""
    o, v = _delta_matrices(old, new)
    n, Ro, Rn = v.shape[0], o.shape[1], v.shape[1]
    m, a = _delta_args(Rn, column_map, always)
    k = n if cap is None else min(int(cap), n)
    rows = np.zeros(k, dtype=np.uint64)
    vr = np.zeros((k, Rn), dtype=np.uint8) if with_verdicts else None
    t = load().kpe_changed_rows_host(o.ctypes.data if o.size else None, v.ctypes.data if v.size else None, n, Ro, Rn,
                                     m.ctypes.data, a.ctypes.data, rows.ctypes.data if k else None,
                                     vr.ctypes.data if (vr is not None and vr.size) else None, k)
    if t < 0:
        check(-t)
    k = min(int(t), k)
    return rows[:k], (vr[:k] if with_verdicts else np.zeros((0, Rn), dtype=np.uint8)), int(t)


def delta_transitions(old, new, column_map) -> np.ndarray:
    """Per new rule the 8 x 8 table [old code, new code] of rows (kpe_delta_transitions_host; no
    device call): (Rn, 8, 8) uint64; old is KPE_NA for a rule column_map maps to -1."""
    o, v = _delta_matrices(old, new)
    n, Ro, Rn = v.shape[0], o.shape[1], v.shape[1]
    m, _ = _delta_args(Rn, column_map, 0)
    out = np.zeros((Rn, 8, 8), dtype=np.uint64)
    check(load().kpe_delta_transitions_host(o.ctypes.data if o.size else None, v.ctypes.data if v.size else None, n,
                                            Ro, Rn, m.ctypes.data, out.ctypes.data if Rn else None))
    return out


def splice_plan(kept_names: Sequence[str], sub_names: Sequence[str], removed: Sequence[str] = ()):
    """The plan of kpe_results_splice from two lists of "<policy>/<rule>" names and the removed
    policies' names, written out in Python: (plan, partner), both int32. plan[r] is the kept column
    that column r of the new kept matrix copies, or -1 - s for column s of sub; partner[s] is the
    kept column named like column s of sub, or -1. An edited policy's columns stand where its first
    kept column stood, in sub's order; added policies are appended. KPE_E_INVALID for a name that
    occurs twice on either side or a removed policy sub also holds, as there."""
    kept = {}
    for i, nm in enumerate(kept_names):
        if nm in kept:
            raise KpeError(1, f"kept rule name occurs twice: {nm}")
        kept[nm] = i
    if len(set(sub_names)) != len(sub_names):
        raise KpeError(1, "rule name occurs twice")
    pol = lambda nm: nm.split("/", 1)[0]
    by_policy = {}  # in sub's order (dicts keep insertion order)
    for s, nm in enumerate(sub_names):
        by_policy.setdefault(pol(nm), []).append(s)
    gone = set(removed)
    if gone & set(by_policy):
        raise KpeError(1, "removed policy is also edited")
    plan, emitted = [], set()
    for c, nm in enumerate(kept_names):
        p = pol(nm)
        if p in by_policy:
            if p not in emitted:
                emitted.add(p)
                plan += [-1 - s for s in by_policy[p]]
        elif p not in gone:
            plan.append(c)
    for p, cols in by_policy.items():
        if p not in emitted:
            plan += [-1 - s for s in cols]
    return np.array(plan, dtype=np.int32), np.array([kept.get(nm, -1) for nm in sub_names], dtype=np.int32)


def splice_names(kept_names: Sequence[str], sub_names: Sequence[str], plan) -> List[str]:
    """The rule names of the spliced matrix: kept names for copied columns, sub's for the others."""
    return [kept_names[int(e)] if e >= 0 else sub_names[-1 - int(e)] for e in plan]


def splice_results(kept, sub, plan, partner, always=0):
    """kpe_results_splice over matrices the caller holds (kpe_results_splice_host; no device call):
    kept (n, Ro), sub (n, Rs), plan and partner as splice_plan gives them, always a mask of
    kpe_verdict bits (SEL(v)) per column of sub or one for all. Returns (the new kept matrix (n, rn)
    uint8, the row flags (n,) uint8 of 0 / 1, the number of changed rows)."""
    k, e = _delta_matrices(kept, sub)
    n, Ro, Rs = k.shape[0], k.shape[1], e.shape[1]
    pl = np.ascontiguousarray(plan, dtype=np.int32)
    rn = pl.shape[0]
    pa, a = _delta_args(Rs, partner, always)
    out = np.zeros((n, rn), dtype=np.uint8)
    flags = np.zeros(max(n, 1), dtype=np.uint8)
    t = load().kpe_results_splice_host(k.ctypes.data if k.size else None, e.ctypes.data if e.size else None, n, Ro, Rs, rn,
                                       pl.ctypes.data if rn else None, pa.ctypes.data, a.ctypes.data,
                                       out.ctypes.data if out.size else None, flags.ctypes.data)
    if t < 0:
        check(-t)
    return out, flags[:n], int(t)


def splice_bytes(n: int, Ro: int, Rs: int, rn: int) -> float:
    """The algorithmic bytes of the splice pass: n x (Ro + Rs + rn + 1) (kpe_splice_bytes)."""
    return float(load().kpe_splice_bytes(n, Ro, Rs, rn))


GATHER_MATRIX, GATHER_FINGERPRINTS = 1, 2  # include/kpe.h KPE_GATHER_*: what Engine.gather_results carries
FP_MASKS = 1  # include/kpe.h KPE_FP_MASKS: FAIL cells' check mask words count
NSL_REPLACE = 1  # include/kpe.h KPE_NSL_REPLACE: the JSON is the whole namespace label table
MESSAGE_CODES = SEL(2) | SEL(4) | SEL(5)  # FAIL, ERROR, SKIP: results whose message the policy text decides


def _ptr(a):
    return None if a is None else a.ctypes.data


def _fp_salts(R: int, salts, msg_salts, msg_codes):
    """(salts or None, msg_salts or None, msg_codes) as the C calls take them."""
    def one(x, what):
        if x is None:
            return None
        a = np.ascontiguousarray(x, dtype=np.uint64)
        if a.shape != (R,):
            raise ValueError(f"{what}: one uint64 per rule")
        return a if R else np.zeros(1, dtype=np.uint64)

    mc = MESSAGE_CODES if msg_codes is None else int(msg_codes)
    if not 0 <= mc <= 0xFF:
        raise ValueError("msg_codes: one byte of SEL(v) bits")
    return one(salts, "salts"), one(msg_salts, "msg_salts"), mc


def rule_salts(ps: PolicySet) -> np.ndarray:
    """The default fingerprint salts of ps's rules (kpe_fp_rule_salts): mix64 of the FNV-1a-64 hash
    of each "<policy>/<rule>" name, never 0. (R,) uint64; XOR a policy's resourceVersion or an edit
    counter into its rules' entries to make the msg_salts of row_fingerprints."""
    out = np.zeros(ps.num_rules, dtype=np.uint64)
    check(load().kpe_fp_rule_salts(ps.h, out.ctypes.data if out.size else None))
    return out


def row_fingerprints(verdicts, salts, msg_salts=None, msg_codes=None, cv_masks=None) -> np.ndarray:
    """The fingerprint of each row of an (n, R) verdict matrix the caller holds
    (kpe_row_fingerprints_host; no device call): (n,) uint64, 0 for a row without responses. salts:
    one per rule; msg_salts / msg_codes as Engine.row_fingerprints; cv_masks: the (n, R) words of
    Engine.cv_masks(raw=True), whose FAIL cells then count (KPE_FP_MASKS)."""
    v = np.ascontiguousarray(verdicts, dtype=np.uint8)
    if v.ndim == 1:
        v = v.reshape(1, -1)
    if v.ndim != 2:
        raise ValueError("verdicts: rows of one cell per rule")
    n, R = v.shape
    s, ms, mc = _fp_salts(R, salts, msg_salts, msg_codes)
    if s is None:
        raise ValueError("salts: one uint64 per rule (rule_salts(ps))")
    m = None
    if cv_masks is not None:
        m = np.ascontiguousarray(cv_masks, dtype=np.uint32).reshape(v.shape)
    out = np.zeros(n, dtype=np.uint64)
    check(load().kpe_row_fingerprints_host(R, v.ctypes.data if v.size else None, _ptr(m) if v.size else None, n, _ptr(s),
                                           _ptr(ms), mc, FP_MASKS if m is not None else 0,
                                           out.ctypes.data if n else None))
    return out


def changed_fingerprints(old, new, cap: Optional[int] = None) -> np.ndarray:
    """The rows whose fingerprints differ (kpe_changed_fingerprints_host): uint64, ascending; at most
    cap of them."""
    a, b = np.ascontiguousarray(old, dtype=np.uint64), np.ascontiguousarray(new, dtype=np.uint64)
    if a.ndim != 1 or a.shape != b.shape:
        raise ValueError("old, new: one fingerprint per row, the same rows")
    k = a.size if cap is None else min(int(cap), a.size)
    rows = np.zeros(k, dtype=np.uint64)
    t = load().kpe_changed_fingerprints_host(a.ctypes.data if a.size else None, b.ctypes.data if b.size else None, a.size,
                                             rows.ctypes.data if k else None, k)
    if t < 0:
        check(-t)
    return rows[:min(int(t), k)]


def cli_summary(ps: PolicySet, counts: List[dict], audit_warn: bool = False) -> Dict[str, int]:
    """`kyverno apply` pass/fail/warn/error/skip totals (processor/result.go:34-68) from the
    per-rule counts Engine.evaluate returns, through kpe_cli_summary."""
    arr = (Counts * max(len(counts), 1))()
    for i, c in enumerate(counts):
        arr[i].na, arr[i].pass_, arr[i].fail = c["na"], c["pass"], c["fail"]
        arr[i].warn, arr[i].error, arr[i].skip = c["warn"], c["error"], c["skip"]
        arr[i].undecided = c.get("undecided", 0)
    out = CliTotals()
    check(load().kpe_cli_summary(ps.h, arr, 1 if audit_warn else 0, ctypes.byref(out)))
    return {"pass": out.pass_, "fail": out.fail, "warn": out.warn, "error": out.error, "skip": out.skip}


NS_COUNT_FIELDS = ("pass", "fail", "warn", "error", "skip", "undecided")  # kpe_ns_counts, in order


def _ns_window(corpus: Corpus, g0: int, ng: Optional[int]) -> int:
    if g0 < 0 or (ng is not None and ng < 0):
        raise ValueError("namespace window: g0 and ng are not negative")
    return max(int(load().kpe_corpus_num_namespaces(corpus.h)) - g0, 0) if ng is None else int(ng)


def namespace_counts(ps: PolicySet, corpus: Corpus, verdicts, g0: int = 0, ng: Optional[int] = None) -> np.ndarray:
    """Engine.namespace_counts over an (n, R) verdict matrix the caller holds (n = the corpus's
    rows), through kpe_namespace_counts_host (no device call): (ng, R, 6) uint32."""
    v = np.ascontiguousarray(verdicts, dtype=np.uint8)
    R = ps.num_rules
    if v.shape != (corpus.n, R):
        raise ValueError("verdicts: one row per resource of the corpus, one cell per rule")
    n = _ns_window(corpus, g0, ng)
    out = np.zeros((n, R, 6), dtype=np.uint32)
    check(load().kpe_namespace_counts_host(ps.h, corpus.h, v.ctypes.data if v.size else None, g0, n,
                                           out.ctypes.data if n else None))
    return out


def cli_summary_ns(ps: PolicySet, corpus: Corpus, counts, audit_warn: bool = False) -> Dict[str, int]:
    """`kyverno apply` totals (processor/result.go:34-68) from the (G, R, 6) per-namespace table of
    every group of the corpus, the action resolved per namespace (kpe_cli_summary_ns): answers
    --audit-warn for policies with validationFailureActionOverrides, which cli_summary refuses."""
    k = np.ascontiguousarray(counts, dtype=np.uint32)
    G = int(load().kpe_corpus_num_namespaces(corpus.h))
    if k.shape != (G, ps.num_rules, 6):
        raise ValueError("counts: (namespaces of the corpus, rules, 6)")
    out = CliTotals()
    buf = k if k.size else np.zeros(6, dtype=np.uint32)
    check(load().kpe_cli_summary_ns(ps.h, corpus.h, buf.ctypes.data, 1 if audit_warn else 0, ctypes.byref(out)))
    return {"pass": out.pass_, "fail": out.fail, "warn": out.warn, "error": out.error, "skip": out.skip}
