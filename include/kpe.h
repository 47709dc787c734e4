/*
 * kpe — MI355X-native batch policy evaluation for Kyverno's validate path.
 *
 * C-ABI drop-in boundary (plain pointers and sizes; no C++/torch types).
 * The reference has no FFI: these entry points are what a cgo shim behind
 * Kyverno's engine interfaces binds:
 *
 *   engineapi.Engine.Validate(ctx, PolicyContext) EngineResponse
 *       pkg/engine/api/engine.go:17-23, implemented by engine.Validate
 *       pkg/engine/engine.go:87-101 (rule loop pkg/engine/validation.go:16-80)
 *     -> kpe_evaluate() answers every (resource, rule) cell of a batch at once;
 *        the Go shim slices one row per PolicyContext.
 *   handlers.Handler.Process (validatePssHandler)
 *       pkg/engine/handlers/handler.go:13-23,
 *       pkg/engine/handlers/validation/validate_pss.go:31-112
 *     -> PSS rules of the compiled program (kpe_check_masks gives the failing
 *        PSA check IDs that become PodSecurityChecks / report "controls").
 *   autogen.ComputeRules  pkg/autogen/autogen.go:236-270
 *     -> kpe_program_compile() runs autogen once, at compile time.
 *   callers: cmd/cli/kubectl-kyverno/processor/policy_processor.go:168-179
 *            (kyverno apply loop) and pkg/controllers/report/utils/scanner.go:99-110
 *            (background scan) build one PolicyContext per (resource, policy);
 *            kpe_corpus_flatten() + kpe_evaluate() replace that loop for a batch.
 *
 * Verdict cell alphabet (engineapi.RuleStatus, pkg/engine/api/rulestatus.go:4-21;
 * "no RuleResponse" = not applicable):
 */
#ifndef KPE_H_
#define KPE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum kpe_verdict {
  KPE_NA = 0,    /* rule did not match the resource: no RuleResponse      */
  KPE_PASS = 1,  /* RuleStatusPass                                         */
  KPE_FAIL = 2,  /* RuleStatusFail                                         */
  KPE_WARN = 3,  /* RuleStatusWarn (reserved; never produced by validate)  */
  KPE_ERROR = 4, /* RuleStatusError (e.g. typed decode failure in getSpec) */
  KPE_SKIP = 5,  /* RuleStatusSkip                                         */
  KPE_UNDECIDED = 7 /* the device could not decide this cell (a documented device limit,
                       e.g. a condition list longer than the VM's list capacity, a resource
                       string that may be JSON where an operator would decode it): the
                       caller evaluates this (resource, rule) with the reference engine */
};

/* Library status codes (0 = OK). Library-level failures set kpe_last_error(). */
typedef int kpe_status;
enum {
  KPE_OK = 0,
  KPE_E_INVALID = 1,     /* malformed input (policy / resource JSON)             */
  KPE_E_UNSUPPORTED = 2, /* policy uses a construct this engine does not evaluate */
  KPE_E_DEVICE = 3,      /* HIP runtime error / no device / kernel not loadable   */
  KPE_E_LIMIT = 4,       /* a corpus exceeds a documented encoding limit          */
  KPE_E_STATE = 5        /* wrong call order (e.g. corpus not uploaded)           */
};

typedef struct kpe_device kpe_device;   /* one HIP device + stream               */
typedef struct kpe_program kpe_program; /* compiled policy set (after autogen)    */
typedef struct kpe_corpus kpe_corpus;   /* flattened, string-interned resources   */

/* Per-rule totals over a batch (pkg/engine/api/policyresponse.go:10-21 counting,
 * cmd/cli/kubectl-kyverno/processor/result.go:34-68 summary line). */
typedef struct kpe_counts {
  uint64_t na, pass, fail, warn, error, skip, undecided;
} kpe_counts;

/* Thread-local message for the last failing call on this thread. */
const char* kpe_last_error(void);
const char* kpe_version(void);

/* ---- device ------------------------------------------------------------ */
kpe_status kpe_device_open(int ordinal, kpe_device** out);
void kpe_device_close(kpe_device* dev);

/* ---- policies ---------------------------------------------------------- */
/* policies_json: one ClusterPolicy/Policy object or a JSON array of them
 * (kyverno.io/v1 schema, api/kyverno/v1/spec_types.go:240-284). Autogen is
 * applied (autogen.ComputeRules). Rules are laid out policy-major, in
 * ComputeRules order: column r of the verdict matrix is rule r.
 * The JMESPath of {{ }} variables and foreach lists includes filter steps `<chain>[?P]` over a
 * single value (P: comparators, `!`, `&&`, `||`, parentheses over element-relative chains, `@` and
 * scalar literals, and contains / starts_with / ends_with with contains(keys(x), 'name')), followed
 * by the steps that may follow `[*]`; a filter's own element list is a result only as a foreach
 * list. Anything outside the device subset is KPE_E_UNSUPPORTED. A filter
 * that keeps more than 32 elements, or compares two arrays / two objects, leaves the cell
 * KPE_UNDECIDED. */
kpe_status kpe_program_compile(const char* policies_json, size_t len, kpe_program** out);
/* kpe_program_compile with PolicyExceptions (kyverno.io/v2beta1, api/kyverno/v2beta1/
 * policy_exception_types.go; the exception lister of engine.NewEngine, pkg/engine/exceptions.go:12-35,
 * consulted per rule at engine.go:286-293): exceptions_json is one PolicyException or a JSON array
 * (NULL / 0: none). A matched cell of a rule an exception names (policyName = the policy key,
 * ruleNames = go-wildcard globs) becomes KPE_SKIP when the exception's match block holds for the
 * resource (pkg/engine/utils/exceptions.go:14-47, validate_resource.go:43-56, validate_pss.go:45-58).
 * KPE_COMPILE_BACKGROUND drops exceptions with spec.background: false, as the background scanner's
 * FetchPolicyExceptions does (pkg/controllers/report/utils/utils.go:113-124); kyverno apply uses
 * every exception it is given. An exception with podSecurity controls re-evaluates a failing pod
 * under them (validate_pss.go:88-104); `conditions` that read the resource, and exceptions on rules
 * whose preconditions read it, are applied after the preconditions (exceptions.go:33-41).
 * KPE_E_UNSUPPORTED: several exceptions on one rule when one has podSecurity controls or
 * conditions that do not fold to true (the first matching one decides). */
#define KPE_COMPILE_BACKGROUND 1u
kpe_status kpe_program_compile_ex(const char* policies_json, size_t len, const char* exceptions_json, size_t exc_len,
                                  uint32_t flags, kpe_program** out);
int kpe_program_num_rules(const kpe_program* prog);
/* "<policy-name>/<rule-name>" of rule r (owned by prog). */
const char* kpe_program_rule_name(const kpe_program* prog, int r);
/* 1 if rule r is a podSecurity rule (check masks are meaningful for it). */
int kpe_program_rule_is_pss(const kpe_program* prog, int r);
void kpe_program_free(kpe_program* prog);

/* ---- resources --------------------------------------------------------- */
/* ndjson: one resource JSON object per line. ns_labels_json: optional
 * {"<namespace>": {"k": "v", ...}, ...} (the namespace label table the
 * reference reads per resource: PolicyContext.NamespaceLabels). */
kpe_status kpe_corpus_flatten(const char* ndjson, size_t len, const char* ns_labels_json, size_t ns_len,
                              kpe_corpus** out);
/* Same with flags. KPE_CORPUS_DOCS keeps every resource's document tape (its JSON as the
 * reference's unstructured map, pkg/engine/validate/validate.go:31 walks it) for
 * pattern / anyPattern rules; kpe_corpus_flatten sets it. Without it the corpus only
 * serves podSecurity and match-only programs (KPE_E_STATE otherwise). */
#define KPE_CORPUS_DOCS 1u
kpe_status kpe_corpus_flatten_ex(const char* ndjson, size_t len, const char* ns_labels_json, size_t ns_len,
                                 uint32_t flags, kpe_corpus** out);
int64_t kpe_corpus_num_resources(const kpe_corpus* c);
/* Host bytes of the columnar encoding (what one evaluation may read). */
int64_t kpe_corpus_bytes(const kpe_corpus* c);
/* 64-bit digest of every column and dictionary of the encoding (identity of two flattens of
 * the same input, e.g. the parallel flattener against a one-thread flatten). */
uint64_t kpe_corpus_digest(const kpe_corpus* c);
/* Per-row status of the flatten (host only, no device call): out[i] for each of the
 * kpe_corpus_num_resources rows. KPE_ROW_DECODE_ERROR: the typed decode of getSpec
 * (validate_pss.go:137-188, encoding/json into corev1.Pod / appsv1.Deployment /
 * batchv1.CronJob) would fail, so every podSecurity cell of the row is a RuleError.
 * KPE_ROW_LIMIT: past a per-resource encoding limit, every cell is KPE_UNDECIDED.
 * KPE_ROW_NO_SPEC: a kind getSpec does not decode ("could not find correct resource type"). */
#define KPE_ROW_DECODE_ERROR 1u
#define KPE_ROW_LIMIT 2u
#define KPE_ROW_NO_SPEC 4u
/* KPE_ROW_CONTEXT_ERROR: NewPolicyContext fails for the resource (AddImageInfos: an invalid image
 * reference or container entry, policycontext/policy_context.go:230), so the reference engine
 * gives no response for any rule and the scanner records an error; every cell is KPE_UNDECIDED. */
#define KPE_ROW_CONTEXT_ERROR 8u
kpe_status kpe_corpus_row_flags(const kpe_corpus* c, uint32_t* out);
/* Resource hash of incremental background scans: CalculateResourceHash
 * (pkg/utils/report/metadata.go:137-155), md5 of json.Marshal([labels, annotations, the object
 * without metadata / status / scale / spec.nodeName]) as 32 lower-case hex digits + NUL in out33.
 * The background controller rescans a resource when it differs from the hash its report
 * recorded (pkg/controllers/report/background/controller.go:247-297). Host only. */
kpe_status kpe_resource_hash(const char* resource_json, size_t len, char* out33);
/* The hash of every NDJSON row (the rows kpe_corpus_flatten makes), 32 hex digits per row into
 * out (no NUL), on up to 16 threads. out == NULL: returns the row count. Returns the row count,
 * or -KPE_E_INVALID when cap_rows is too small. A row that is not a JSON object (which the
 * flattener keeps with KPE_ROW_DECODE_ERROR) has no hash: its 32 bytes are '-' (never a hex
 * digest), so an incremental scan always re-evaluates it. */
int64_t kpe_resource_hashes(const char* ndjson, size_t len, char* out, int64_t cap_rows);
/* Namespace groups of the corpus (host only, no device call). A resource's group is the namespace
 * the flattener recorded as its metadata.namespace, i.e. unstructured GetNamespace(), the value
 * GetValidationFailureAction (pkg/engine/api/engineresponse.go:196-225) compares and the key of the
 * CLI's NamespaceSelectorMap (cmd/cli/kubectl-kyverno/processor/policy_processor.go:63). It is not
 * the match namespace: a `kind: Namespace` object groups under "" like every cluster-scoped
 * resource, not under its own name. Group ids are dense in [0, G) and fixed for the corpus's
 * lifetime (the ids of its namespace dictionary, which also holds the names of Namespace objects:
 * a group may have no rows). The group "" always exists; a row without a namespace string (no
 * metadata.namespace, or a row whose recorded id is outside the dictionary, such as KPE_NO_STR)
 * belongs to it. kpe_corpus_flatten refuses a line that is not a JSON object, so no row lacks a
 * recorded id today. */
int64_t kpe_corpus_num_namespaces(const kpe_corpus* c);
/* Name of group g (owned by the corpus; NULL when g is out of range). */
const char* kpe_corpus_namespace(const kpe_corpus* c, int64_t g);
/* out[i] = the group of row i, for each of the kpe_corpus_num_resources rows. */
kpe_status kpe_corpus_row_namespaces(const kpe_corpus* c, uint32_t* out);
/* out[g] = the rows of group g (G entries; their sum is N). The KPE_NA cells of a (group, rule)
 * are these rows minus the six counters of kpe_ns_counts. Retired rows (kpe_corpus_retire_rows)
 * are still counted here: every cell of theirs is KPE_NA, so the statement holds for them too. */
kpe_status kpe_corpus_namespace_rows(const kpe_corpus* c, uint64_t* out);
/* Copy the columns to device memory (HBM). Evaluation requires this. */
kpe_status kpe_corpus_upload(kpe_device* dev, kpe_corpus* c);
/* Retire rows of a corpus (a resource that was deleted, or replaced by a row of another corpus):
 * from the next evaluation on, every cell of a retired row is KPE_NA and every check-mask word of
 * it 0, in every form of evaluation (kpe_evaluate, kpe_evaluate_async[_ex], kpe_evaluate_batch_async
 * and its multi-shard launches, kpe_evaluate_sharded; with and without KPE_EVAL_MASKS /
 * KPE_EVAL_COLD), before any consumer reads: the fetches, counts, selections, summaries, namespace
 * counts, kept results and deltas, fingerprints (0, "no report", for a retired row), report rows,
 * packed and device verdicts and the traces all see a row without responses. Retirement overrides
 * whatever the row would otherwise be (KPE_UNDECIDED of a row past a limit or with a context error,
 * a decode-error KPE_ERROR, an applyRules: One outcome). Results of an evaluation that was already
 * enqueued, and kept results, stay as they are.
 * The set only grows (union; duplicates and any order allowed), belongs to the corpus until
 * kpe_corpus_free and survives kpe_corpus_upload, which sends it again. dev may be NULL for a corpus
 * that is not uploaded: the set is recorded on the host and travels with the next upload. For an
 * uploaded corpus the device list is refreshed on the corpus's stream, ordered before its next
 * evaluation. KPE_E_INVALID for a row >= N or a null rows with n > 0; KPE_E_STATE for an uploaded
 * corpus with a null device or a device other than its own; both checked before any device call,
 * and the set is then left untouched. */
kpe_status kpe_corpus_retire_rows(kpe_device* dev, kpe_corpus* c, const uint64_t* rows, uint64_t n);
/* The retired rows, ascending and unique: the first min(total, cap) into rows[]; returns the total
 * (rows == NULL with cap == 0 counts only), or -kpe_status. Host only. */
int64_t kpe_corpus_retired_rows(const kpe_corpus* c, uint64_t* rows, uint64_t cap);
/* Change the namespace label table of a flattened corpus in place (the labels of a Namespace
 * changed; the reference reads them fresh at every rescan, background/controller.go:310-318).
 * flags == 0 is a patch: every member "<namespace>": {...} of the JSON object sets that
 * namespace's entry, its value read as kpe_corpus_flatten reads ns_labels_json (string-valued
 * members are the labels, other members are skipped, a value that is no object gives an entry
 * without labels); "<namespace>": null removes the entry; namespaces not named keep theirs; a key
 * that occurs twice counts by its last occurrence; a null or empty argument changes nothing.
 * KPE_NSL_REPLACE: the table becomes what kpe_corpus_flatten builds from this JSON (null, empty or
 * {}: no table).
 * After the call every consumer behaves as on a corpus flattened from the same NDJSON with the
 * resulting table: verdicts, check masks, counts, namespace counts, kpe_cli_summary_ns, row
 * summaries, fingerprints, report rows and traces. kpe_corpus_digest is not part of that: new label
 * strings are appended to the label dictionaries, where a fresh flatten interns the table first, so
 * the ids, and with them the digest, differ from a fresh corpus's. A namespace without an entry and
 * one whose entry has no labels are the same to every consumer, before and after.
 * *changed (may be NULL) receives the number of namespaces whose entry changed, labels compared as
 * sets of (key, value) pairs. When it is 0 nothing is touched or invalidated.
 * Otherwise the call waits for the corpus's last evaluation and leaves the corpus without one:
 * the fetch, select and trace calls answer KPE_E_STATE until the next evaluation, which binds the
 * program again in full. Kept results, kept fingerprints, the retired rows and the namespace groups
 * (kpe_corpus_num_namespaces, kpe_corpus_row_namespaces: a namespace that only the table names is
 * no group) stay. dev may be NULL for a corpus that is not uploaded: the table changes on the host
 * and travels with the next upload. On an uploaded corpus the table (and the label dictionaries
 * when they grew) are sent again on the corpus's stream and every row's table row is recomputed on
 * the device from its namespace id; nothing proportional to the rows crosses the bus.
 * KPE_E_INVALID for malformed JSON or a top level that is no object; KPE_E_STATE for an uploaded
 * corpus with a null device or a device other than its own; both before anything changes. The call
 * needs exclusive use of the corpus, as kpe_corpus_upload and kpe_corpus_retire_rows do. */
#define KPE_NSL_REPLACE 1u
kpe_status kpe_corpus_set_namespace_labels(kpe_device* dev, kpe_corpus* c, const char* ns_labels_json, size_t len,
                                           uint32_t flags, uint64_t* changed /* may be NULL */);
/* The current table as JSON, {"<namespace>": {"<key>": "<value>", ...}, ...} in table order (given
 * back with KPE_NSL_REPLACE it rebuilds the same table): writes at most cap bytes into out (no
 * terminator) and returns the length needed, or -kpe_status. Host only. */
int64_t kpe_corpus_namespace_labels(const kpe_corpus* c, char* out, size_t cap);
/* A corpus out of chosen rows of other corpora (host only, no JSON is read): pairs is npairs x
 * {src, row}, and row k of *out is row `row` of srcs[src]. Every consumer behaves as on a corpus
 * flattened from the listed rows' NDJSON lines, in list order, under the sources' namespace label
 * table: evaluation in every form (verdicts, check masks, counts), namespace counts, row flags,
 * exclusions, traces, report rows and fingerprints. *out is not uploaded, has nothing retired and
 * keeps nothing. Runs on the flattener's threads.
 * Ids: the sources' dictionaries, scalar tables and capability sets are merged whole, in source
 * order, first occurrence first (the parallel flattener's rule). When every row of every source is
 * listed in source order the ids are those of a sequential flatten: for sources that are consecutive
 * chunks of one NDJSON, kpe_corpus_digest(*out) equals the digest of flattening the whole input. For
 * any other list the digest may differ (strings only dropped rows used stay in the dictionaries, so
 * a namespace group without rows may exist where a fresh flatten has none); no consumer sees ids.
 * Rows: a row listed twice appears twice. A row that is KPE_ROW_LIMIT in its source stays so (some
 * limits depend on the source's dictionaries; KPE_UNDECIDED is the safe side), so equality with a
 * fresh flatten holds for rows not past a limit in their source. The decode-error, no-spec and
 * context-error flags travel with the row.
 * KPE_E_INVALID: a null argument or nsrcs < 1; a pair outside its source or naming a retired row;
 * sources that differ in KPE_CORPUS_DOCS; sources whose namespace label tables differ (compared by
 * namespace, as sets of pairs). KPE_E_LIMIT: the merged dictionaries or capability sets cross a
 * corpus-wide or per-resource limit the sources' rows were flattened under, or a column outgrows its
 * 32-bit offsets: flatten the lines again. On any error *out is untouched. */
kpe_status kpe_corpus_gather(const kpe_corpus* const* srcs, int nsrcs, const uint64_t* pairs, uint64_t npairs,
                             kpe_corpus** out);
/* One 64-bit digest per row that holds no id and no position (host only; out: N words): every
 * dictionary id stands by its string, a GVK by its three strings, a capability mask by its names, a
 * capability-set id by its (add, drop) sets, a scalar id by its type, value bits and texts, the row's
 * label-table row by that namespace's label pairs as a set, and the document tape is walked from the
 * row's root and its `images` root with every kind and count word. Two corpora give a row the same
 * digest whenever it was flattened from the same line under the same label table, whatever else they
 * hold; it changes when any word of the row that the kernels, the exclusion pass, the traces or the
 * reports read changes. The check of kpe_corpus_gather, and a diagnostic for a resident corpus
 * against its NDJSON. */
kpe_status kpe_corpus_row_digests(const kpe_corpus* c, uint64_t* out);
/* The corpus's per-pod PSA summary, built on dev (waits for it; builds it first when no LEAN
 * evaluation has yet): 2 words per row (include-free layout of kyverno_amd/csrc/schema.h PS_*:
 * x = OR of the pod's container state bitmaps, y = the list codes under the PSA library's fixed
 * sets). Diagnostics and the summary's digest test; evaluation never needs it on the host. */
kpe_status kpe_corpus_psa_summary(kpe_device* dev, kpe_corpus* c, uint32_t* out);
void kpe_corpus_free(kpe_corpus* c);

/* ---- evaluation -------------------------------------------------------- */
/* Evaluate every (resource, rule) cell on the device and copy results back.
 *   verdicts    : N x R bytes (row-major, kpe_verdict), may be NULL
 *   check_masks : N x R uint32 (bit k = PSA check k failed, kpe_pss_check_id
 *                 order; 0 for non-PSS rules), may be NULL
 *   counts      : R entries, may be NULL
 * Synchronous. Safe to call from several OS threads on distinct devices; calls
 * on one device are serialised by a per-device mutex. */
kpe_status kpe_evaluate(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, uint8_t* verdicts,
                        uint32_t* check_masks, kpe_counts* counts);

/* Asynchronous form for pipelines/benchmarks: enqueue one evaluation on the
 * device stream; results stay in device buffers owned by the corpus. No host
 * synchronisation. Use kpe_device_sync() and kpe_fetch() afterwards. */
kpe_status kpe_evaluate_async(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c);
/* kpe_evaluate_async with options: KPE_EVAL_MASKS also writes the check masks (device
 * buffers read by kpe_fetch / kpe_fetch_cv_masks); KPE_EVAL_COLD re-runs the binding's
 * per-corpus prologue (dictionary predicate pass, prologue image and, for a LEAN program, the
 * per-pod PSA summaries) as the first evaluation of a newly bound corpus does. */
#define KPE_EVAL_MASKS 1u
#define KPE_EVAL_COLD 2u
kpe_status kpe_evaluate_async_ex(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, unsigned flags);
/* n evaluations enqueued by one call, corpora cs[0 .. n-1] in order (a corpus may repeat), each
 * with the results kpe_evaluate_async_ex(dev, prog, cs[i], flags) gives: the batch form a scanner
 * driving many resident shards (or a benchmark) uses instead of n foreign-function calls. A run of
 * consecutive warm shards whose evaluation is the LEAN evaluation alone (a bound kind-only
 * podSecurity program, no later kernels) goes out as ceil(m / 24) multi-shard launches of
 * kpe_lean6_kernel: one grid over the shards' tiles instead of one launch per shard. Every launch
 * evaluates each pod's PSA checks from its pod, container, volume, sysctl and annotation columns. */
kpe_status kpe_evaluate_batch_async(kpe_device* dev, const kpe_program* prog, const kpe_corpus* const* cs, int n,
                                    unsigned flags);
kpe_status kpe_device_sync(kpe_device* dev);
kpe_status kpe_fetch(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, uint8_t* verdicts,
                     uint32_t* check_masks, kpe_counts* counts);

/* ---- verdict exchange and several devices in one process ---------------- */
/* Device address and size of the corpus's N x R verdict matrix after an evaluation of prog on
 * dev (waits for it): valid until the next evaluation of the corpus. A collective can send it
 * straight from HBM (RCCL over xGMI); SURVEY.md 8(e)'s verdict gather. */
kpe_status kpe_device_verdicts(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, void** dptr,
                               uint64_t* bytes);
/* The verdict matrix packed on the device into 3-bit cells (the kpe_verdict alphabet fits),
 * 10 per 32-bit word, row-major: cell i is bits 3*(i % 10) .. +2 of word i / 10. dst_dev is
 * device memory of dev holding at least kpe_packed_words(N * R) words (e.g. a torch tensor
 * that RCCL then sends); synchronous. kpe_unpack_verdicts expands it on the host. */
uint64_t kpe_packed_words(uint64_t cells);
kpe_status kpe_pack_verdicts(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, uint32_t* dst_dev,
                             uint64_t words);
kpe_status kpe_unpack_verdicts(const uint32_t* packed, uint64_t cells, uint8_t* out);
/* One logical corpus sharded over several devices of this process: shards[i] uploaded to
 * devs[i] (distinct devices), evaluated concurrently; verdicts = the shards' rows in order
 * (sum of N_i x R bytes, may be NULL), counts = the per-rule sums (R entries, may be NULL). The
 * Go host's single-process multi-GPU entry. */
kpe_status kpe_evaluate_sharded(kpe_device* const* devs, kpe_corpus* const* shards, int nshards,
                                const kpe_program* prog, uint8_t* verdicts, kpe_counts* counts);

/* ---- sparse result fetch -------------------------------------------------- */
/* The cells a consumer needs, selected on the device, instead of kpe_fetch's whole N x R matrix
 * and a host walk over it. After kpe_evaluate / kpe_evaluate_async of prog on the corpus (waits for
 * it; KPE_E_STATE without one), like kpe_pack_verdicts.
 *   sel : R bytes; cell (row, r) with verdict v is selected iff (sel[r] >> v) & 1.
 * Writes the first min(total, cap) selected cells in ascending cell index (row * R + r) into
 * cells[] (and their verdict codes into verdicts_out[] when not NULL); memory past that is not
 * written. cells == NULL with cap == 0 counts only. Returns the total number of selected cells
 * (call again with a larger buffer when it exceeds cap), or -kpe_status. cells[] is the list
 * kpe_pattern_traces takes: KPE_SEL(KPE_FAIL) on the pattern rules' columns gives the cells whose
 * failing paths the report needs (validate_resource.go:316-454). KPE_SEL_RESPONSES selects the cells
 * that carry a RuleResponse (every code but KPE_NA), i.e. the cells EngineResponseToReportResults
 * (pkg/utils/report/results.go:89-135) turns into report results, plus KPE_UNDECIDED cells. */
#define KPE_SEL(v) (1u << (v))
#define KPE_SEL_RESPONSES 0xFEu
int64_t kpe_select_cells(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, const uint8_t* sel,
                         uint64_t* cells, uint8_t* verdicts_out, uint64_t cap);

/* The `summary` block of each resource's report: CalculateSummary (pkg/utils/report/results.go:39-55)
 * over the results EngineResponseToReportResults gives (:89-135; SetResponses -> SetResults ->
 * CalculateSummary, :182-196; the CLI per policy, cmd/cli/kubectl-kyverno/report/report.go:93,104).
 * Per row: KPE_PASS counts as pass, KPE_FAIL as fail, or as warn when the rule's policy is unscored
 * (policies.kyverno.io/scored: "false", results.go:131-133), KPE_WARN as warn, KPE_ERROR as error,
 * KPE_SKIP as skip; KPE_NA is not counted. `undecided` (not part of the reference's summary) counts
 * the row's KPE_UNDECIDED cells: non-zero, the row needs the reference engine (kpe_counts.undecided
 * by row). KPE_E_LIMIT for more than 65535 rules (16-bit counters). */
typedef struct kpe_row_summary {
  uint16_t pass, fail, warn, error, skip, undecided;
} kpe_row_summary;
/* Rows [row0, row0 + nrows) of the last evaluation of prog on the corpus, counted on the device
 * (12 bytes per row come back instead of R); KPE_E_INVALID when row0 + nrows > N. */
kpe_status kpe_fetch_row_summaries(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, uint64_t row0,
                                   uint64_t nrows, kpe_row_summary* out);
/* The same fold over nrows x R verdict bytes the caller holds. Host only; no device call. */
kpe_status kpe_row_summaries_host(const kpe_program* prog, const uint8_t* verdicts, uint64_t nrows,
                                  kpe_row_summary* out);

/* ---- result deltas ---------------------------------------------------------- */
/* Which reports change after a policy or PolicyException change. The background controller
 * re-evaluates every resource, keeps the results of unchanged policies (pkg/controllers/report/
 * background/controller.go:379-389,392-419) and writes a report only when it differs from the stored
 * one (storeReport returns on ReportsAreIdentical, controller.go:463, pkg/controllers/report/utils/
 * utils.go:66-88). For a resident corpus: keep the verdict matrix of one evaluation on the device,
 * evaluate the new program, and fetch only the rows that differ.
 *
 * kpe_results_keep: after kpe_evaluate / kpe_evaluate_async of prog on the corpus (KPE_E_STATE
 * without one, like kpe_select_cells), copy the corpus's N x R verdict matrix device to device into a
 * buffer the corpus owns, with R and the rules' "<policy>/<rule>" names (prog may be freed
 * afterwards). The copy is enqueued behind the evaluation and ahead of the corpus's next one, which
 * overwrites the matrix; the call does not wait for it. A kept result replaces the previous one and
 * lives until kpe_results_drop, kpe_corpus_upload or kpe_corpus_free. It costs N x R bytes of device
 * memory (HBM) per kept corpus. */
kpe_status kpe_results_keep(kpe_device* dev, const kpe_program* prog, kpe_corpus* c);
kpe_status kpe_results_drop(kpe_device* dev, kpe_corpus* c);
/* The kept R, or -1 when nothing is kept; the name of kept rule r (owned by the corpus, NULL when
 * r is out of range or nothing is kept). */
int kpe_results_kept_rules(const kpe_corpus* c);
const char* kpe_results_kept_rule_name(const kpe_corpus* c, int r);
/* old_of[r], for every rule r of prog: the kept column whose rule name equals
 * kpe_program_rule_name(prog, r), or -1. KPE_E_STATE when nothing is kept; KPE_E_INVALID for a name
 * that occurs twice among the kept rules or among prog's (the map would be ambiguous: pass one of
 * your own). Host only. */
kpe_status kpe_delta_column_map(const kpe_corpus* c, const kpe_program* prog, int32_t* old_of);
/* The rows of the last evaluation of prog on the corpus (the new matrix, Rn rules) that differ from
 * the kept one (Ro rules). With old(i, r) = kept[i][old_of[r]], or KPE_NA when old_of[r] is -1, row
 * i is changed iff
 *   - new[i][r] != old(i, r) for some new column r, or
 *   - (always[r] >> new[i][r]) & 1 for some new column r (the `sel` convention of kpe_select_cells:
 *     KPE_SEL(KPE_FAIL) | KPE_SEL(KPE_ERROR) | KPE_SEL(KPE_SKIP) on the columns of an edited policy
 *     counts the cells whose message may differ under an equal verdict; PASS and NA cells, whose
 *     report entry is constant, are still compared), or
 *   - a kept column that no old_of[r] names holds a code other than KPE_NA in row i (a rule that
 *     disappeared).
 * old_of: Rn entries, NULL = kpe_delta_column_map; always: Rn bytes, NULL = all zero. Writes the first
 * min(total, cap) changed row indices, ascending, into rows[] and, when verdict_rows is not NULL,
 * those rows of the new matrix (Rn bytes each) into verdict_rows[]; memory past that is not written.
 * rows == NULL with cap == 0 counts only. Returns the total number of changed rows, or -kpe_status:
 * KPE_E_INVALID for a null argument, cap > 0 without rows, an old_of entry below -1 or not below the
 * kept R, or a kept column named twice; KPE_E_LIMIT when either side has more than KPE_DELTA_MAX_RULES
 * rules (the kernel stages the kept rows of a row group and the per-rule tables in LDS); all checked
 * before any device call. KPE_E_STATE when nothing is kept, the corpus has no evaluation of prog, or
 * it is uploaded to another device. */
#define KPE_DELTA_MAX_RULES 4096
int64_t kpe_changed_rows(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, const int32_t* old_of,
                         const uint8_t* always, uint64_t* rows, uint8_t* verdict_rows, uint64_t cap);
/* The comparison across corpora, for the rows a small delta corpus replaces in a resident one.
 * pairs: npairs x {new_row, old_row}. Pair k compares row new_row of the last evaluation of prog on
 * c_new with row old_row of c_old's KEPT matrix, by the rules of kpe_changed_rows (old_of, always,
 * disappeared columns; old_of == NULL maps by rule name against c_old's kept names, as
 * kpe_delta_column_map does). Writes the first min(total, cap) indices k of the changed pairs,
 * ascending, into changed[] and, when verdict_rows is not NULL, their rows of the new matrix (Rn
 * bytes each); memory past that is not written. changed == NULL with cap == 0 counts only. An old_row
 * may occur in several pairs; c_new == c_old is allowed. Returns the total, or -kpe_status:
 * KPE_E_INVALID for a null argument (pairs with npairs > 0), cap > 0 without changed, a pair's row
 * outside its corpus, or a bad column map; KPE_E_LIMIT past KPE_DELTA_MAX_RULES; all checked before
 * any device call. KPE_E_STATE when c_old keeps nothing, c_new has no evaluation of prog, or either
 * corpus is not uploaded to dev. The host form is kpe_changed_rows_host over the gathered rows. */
int64_t kpe_changed_pairs(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c_new, const kpe_corpus* c_old,
                          const uint64_t* pairs, uint64_t npairs, const int32_t* old_of, const uint8_t* always,
                          uint64_t* changed, uint8_t* verdict_rows, uint64_t cap);
/* What a policy edit does to the cluster: per new column r the table out[r * 64 + old * 8 + new] of
 * rows by kept and new verdict code (old = KPE_NA for an unmapped column); a column's table sums to
 * N. out: Rn x 64 counters. Arguments, map and errors as kpe_changed_rows. */
kpe_status kpe_delta_transitions(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, const int32_t* old_of,
                                 uint64_t* out);
/* The same over two matrices the caller holds (old_v: n x Ro, new_v: n x Rn; old_of: Rn entries,
 * required): the specification of the device calls, and what a caller without a resident corpus
 * uses. No rule limit. Host only; no device call. */
int64_t kpe_changed_rows_host(const uint8_t* old_v, const uint8_t* new_v, uint64_t n, uint32_t Ro, uint32_t Rn,
                              const int32_t* old_of, const uint8_t* always, uint64_t* rows, uint8_t* verdict_rows,
                              uint64_t cap);
kpe_status kpe_delta_transitions_host(const uint8_t* old_v, const uint8_t* new_v, uint64_t n, uint32_t Ro, uint32_t Rn,
                                      const int32_t* old_of, uint64_t* out);

/* ---- policy edits on a kept result -------------------------------------------- */
/* One policy edited, added or removed out of hundreds. After a policy change the background
 * controller keeps the stored results of the unchanged policies and recomputes only the changed ones
 * (pkg/controllers/report/background/controller.go:379-419). A rule's verdict depends only on its
 * own policy, the resource, the namespace labels and the exceptions naming that policy, so the
 * columns of a policy compiled alone equal its columns inside the full program: evaluate `sub`, the
 * edited and added policies compiled alone with their exceptions, and splice its N x Rs matrix E
 * into the kept matrix K (N x Ro) instead of evaluating, comparing and keeping all R columns.
 *
 * The plan. Names are "<policy>/<rule>". The new kept matrix K' (N x rn) is the kept columns in
 * order, where a column whose policy is neither in sub nor in `removed` is copied (plan[r] = c); at
 * the first kept column of a policy sub holds, all of sub's columns of that policy follow in sub's
 * order (plan[r] = -1 - s) and the policy's other kept columns are skipped, so an edited policy
 * keeps its place whatever its rule count; the columns of removed policies vanish; the policies of
 * sub not among the kept ones are appended in sub's order. K' takes the kept names of copied columns
 * and kpe_program_rule_name(sub, s) for the others. kpe_splice_plan writes the first min(rn, cap)
 * entries and returns rn, or -kpe_status: KPE_E_INVALID for a null argument, a removed name that sub
 * also holds, or a rule name that occurs twice on either side; KPE_E_STATE when nothing is kept;
 * KPE_E_LIMIT when Ro, Rs or rn is past KPE_DELTA_MAX_RULES. Host only. kpe_splice_plan_names is
 * the same over two name lists (no corpus, no rule limit) and also gives partner[s], the kept
 * column named like column s of sub, or -1 (NULL: not wanted). */
int64_t kpe_splice_plan(const kpe_corpus* c, const kpe_program* sub, const char* const* removed, uint32_t nremoved,
                        int32_t* plan, uint32_t cap);
int64_t kpe_splice_plan_names(const char* const* kept, uint32_t Ro, const char* const* sub, uint32_t Rs,
                              const char* const* removed, uint32_t nremoved, int32_t* plan, int32_t* partner,
                              uint32_t cap);
/* kpe_results_splice: the corpus holds a kept result and its last evaluation is of sub (KPE_E_STATE
 * otherwise, or when it is uploaded to another device; a sub without rules, for an edit that only
 * removes policies, needs no evaluation). One kernel pass, enqueued behind that
 * evaluation and ahead of the corpus's next one on the stream kpe_results_keep uses, writes K' into a
 * second buffer the corpus owns and one flag byte per row; then the two buffers swap and the kept R
 * and names become K''s: kpe_results_kept_rule_name, kpe_delta_column_map, kpe_changed_rows and
 * kpe_changed_pairs see K' like any kept result. Row i is changed (the rule of kpe_changed_rows
 * between K and K', restricted to what can differ; copied columns are equal by construction) iff
 *   - E[i][s] != K[i][p(s)] for some column s of sub, p(s) the kept column of the same name (none:
 *     the cell counts as KPE_NA), or
 *   - (always[s] >> E[i][s]) & 1 for some column s of sub (always: Rs bytes, NULL = all zero), or
 *   - a kept column that is neither copied nor a partner holds a code other than KPE_NA in row i.
 * Returns the number of changed rows (the call waits for the pass), or -kpe_status: the plan's
 * errors, checked before any device call. The old buffer stays as the spare of the next splice and
 * the flags (N bytes) stay until the next splice, keep, drop or upload: a corpus that splices costs
 * up to 2 x N x max(Ro, rn) + N bytes of device memory; kpe_results_drop, kpe_corpus_upload and
 * kpe_corpus_free release all of it. Check masks and traces are not kept across a splice. */
int64_t kpe_results_splice(kpe_device* dev, const kpe_program* sub, kpe_corpus* c, const char* const* removed,
                           uint32_t nremoved, const uint8_t* always /* Rs bytes or NULL */);
/* The changed rows of the last kpe_results_splice on the corpus (KPE_E_STATE without one): the first
 * min(total, cap) row indices, ascending, into rows[] and, when verdict_rows is not NULL, those rows
 * of K' (rn bytes each); memory past that is not written. rows == NULL with cap == 0 counts only.
 * Reads the kept flag bytes; compares nothing again, and may be called repeatedly. Returns the total
 * or -kpe_status. */
int64_t kpe_spliced_rows(kpe_device* dev, const kpe_corpus* c, uint64_t* rows, uint8_t* verdict_rows, uint64_t cap);
/* The same over matrices the caller holds (kept: n x Ro, sub_v: n x Rs; plan: rn entries; partner:
 * Rs entries, -1 = none; always: Rs bytes or NULL): writes out (n x rn) and flags (n bytes of 0 / 1)
 * and returns the number of changed rows, or -KPE_E_INVALID for a null argument, an entry out of
 * range, a kept column copied or partnered twice or both, or a column of sub emitted twice or not at
 * all. The specification of kpe_results_splice. No rule limit. Host only; no device call. */
int64_t kpe_results_splice_host(const uint8_t* kept, const uint8_t* sub_v, uint64_t n, uint32_t Ro, uint32_t Rs,
                                uint32_t rn, const int32_t* plan, const int32_t* partner, const uint8_t* always,
                                uint8_t* out, uint8_t* flags);
/* Rows [row0, row0 + nrows) of the kept matrix (kept R bytes each) to the host: diagnostics and
 * tests. KPE_E_STATE when nothing is kept. */
kpe_status kpe_results_kept_fetch(kpe_device* dev, const kpe_corpus* c, uint64_t row0, uint64_t nrows, uint8_t* out);
/* The splice pass: its algorithmic bytes, N x (Ro + Rs + rn + 1); the rows of one of its row groups
 * and the most groups in flight (blocks of its persistent grid). */
double kpe_splice_bytes(uint64_t n, uint32_t Ro, uint32_t Rs, uint32_t rn);
uint32_t kpe_splice_group_rows(uint32_t Ro, uint32_t Rs, uint32_t rn);
uint32_t kpe_splice_max_groups(void);

/* ---- row fingerprints -------------------------------------------------------- */
/* Report-change detection in 8 bytes per resource. The reference decides "identical or not" from one
 * small thing per report (ReportsAreIdentical, pkg/controllers/report/utils/utils.go:66-88) and stores
 * the resource's hash as a label on it (pkg/utils/report/metadata.go:137-155). A fingerprint is the
 * matching value of a resource's report results: the caller can store it with the report (an
 * annotation), load it back after a restart or a re-upload, and compare on the device, so that only the
 * changed rows come back. A kept matrix (kpe_results_keep) costs N x R bytes and dies with the upload;
 * kept fingerprints cost 8 N bytes and can be restored.
 *
 * All arithmetic is on uint64_t and wraps.
 *   mix64(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31
 * (the splitmix64 finaliser: a bijection, mix64(0) == 0). For row i of an evaluation with R rules
 *   fp(i) = sum over the columns r with v = V[i][r] != KPE_NA of
 *             mix64( S(r, v) + 0x9E3779B97F4A7C15 * ( v | (uint64_t)m(i, r) << 8 ) )
 *   S(r, v)  = msg_salts[r] when (msg_codes >> v) & 1, else salts[r]. msg_codes: one byte in the KPE_SEL
 *              convention; KPE_SEL(KPE_FAIL) | KPE_SEL(KPE_ERROR) | KPE_SEL(KPE_SKIP) names the results
 *              whose message the policy text decides. msg_salts == NULL means salts.
 *   m(i, r)  = the cell's versioned-check mask word, bit 31 (KPE_CVM_XMATCH) included, exactly as
 *              kpe_fetch_cv_masks returns it, when flags & KPE_FP_MASKS and v == KPE_FAIL; else 0. With
 *              KPE_FP_MASKS the evaluation must have written masks (KPE_E_STATE otherwise, as
 *              kpe_fetch_cv_masks).
 * Properties:
 *   - the sum commutes: a column permutation with its salts does not change fp;
 *   - a column that is KPE_NA in the row contributes nothing: an added policy that does not match the
 *     resource leaves its fingerprint, and its report, unchanged;
 *   - fp == 0 for a row without responses (the controller's "no report");
 *   - XOR a policy's resourceVersion (or an edit counter) into msg_salts[r] of its rules: an edit then
 *     changes the fingerprint of exactly the rows with a msg_codes cell in those columns, the job
 *     `always` does for kpe_changed_rows.
 * A fingerprint is a hash: two different result sets of a row collide with probability 2^-64 per
 * comparison. kpe_changed_rows against a kept matrix remains the exact form.
 *
 * More than KPE_DELTA_MAX_RULES rules is KPE_E_LIMIT for the device calls (checked before the state;
 * the host twins have no limit). Argument checks come before any device call; the state rules are those
 * of kpe_fetch_row_summaries. */
#define KPE_FP_MASKS 1u
/* salts[r] = mix64(FNV-1a-64("<policy>/<rule>")), 0 replaced by 1: the default salts, R entries. Host
 * only. */
kpe_status kpe_fp_rule_salts(const kpe_program* prog, uint64_t* salts);
/* The fingerprints of rows [row0, row0 + nrows) of the last evaluation of prog on the corpus.
 * salts == NULL: the default salts. KPE_E_INVALID when row0 + nrows > N, for a null argument or an
 * unknown flag; nrows == 0 writes nothing. */
kpe_status kpe_fetch_row_fingerprints(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c,
                                      const uint64_t* salts, const uint64_t* msg_salts, uint8_t msg_codes,
                                      uint32_t flags, uint64_t row0, uint64_t nrows, uint64_t* out);
/* The same over nrows x R verdict bytes (and, with KPE_FP_MASKS, nrows x R mask words) the caller holds:
 * the plain double loop, the specification of the device call, and what a caller without a resident
 * corpus uses. salts is required; cv_masks may be NULL without KPE_FP_MASKS. Host only; no rule limit. */
kpe_status kpe_row_fingerprints_host(uint32_t R, const uint8_t* verdicts, const uint32_t* cv_masks, uint64_t nrows,
                                     const uint64_t* salts, const uint64_t* msg_salts, uint8_t msg_codes,
                                     uint32_t flags, uint64_t* out);
/* Compute the fingerprints of the last evaluation of prog on the corpus into an 8 x N byte buffer the
 * corpus owns. Enqueued behind the evaluation, as kpe_results_keep is; does not wait. Kept fingerprints
 * replace the previous ones and live until kpe_fingerprints_drop, kpe_corpus_upload or
 * kpe_corpus_free; they are independent of the kept matrix, and both may exist at once. */
kpe_status kpe_fingerprints_keep(kpe_device* dev, const kpe_program* prog, kpe_corpus* c, const uint64_t* salts,
                                 const uint64_t* msg_salts, uint8_t msg_codes, uint32_t flags);
/* Restore stored fingerprints as the kept ones (n must equal N: KPE_E_INVALID otherwise; KPE_E_STATE
 * when the corpus is not uploaded to dev). */
kpe_status kpe_fingerprints_load(kpe_device* dev, kpe_corpus* c, const uint64_t* fp, uint64_t n);
/* Rows [row0, row0 + nrows) of the kept fingerprints (waits for a pending keep); KPE_E_STATE when
 * nothing is kept. */
kpe_status kpe_fingerprints_fetch(kpe_device* dev, const kpe_corpus* c, uint64_t row0, uint64_t nrows, uint64_t* out);
kpe_status kpe_fingerprints_drop(kpe_device* dev, kpe_corpus* c);
int kpe_fingerprints_kept(const kpe_corpus* c); /* 0 or 1 */
/* Carry kept results into a gathered corpus (kpe_corpus_gather), on the device: dst, uploaded to dev
 * with npairs rows, receives as its kept matrix (KPE_GATHER_MATRIX) row k = kept row `row` of
 * srcs[src], with the sources' R and rule names, and as its kept fingerprints
 * (KPE_GATHER_FINGERPRINTS) the 8 bytes of the same rows; what == 0 carries whatever every listed
 * source keeps (possibly nothing). A source is listed when a pair names it (every source when
 * npairs == 0). No evaluation and no program are involved; whatever dst kept of a requested kind is
 * replaced. The copy is ordered after each listed source's pending kpe_results_keep /
 * kpe_fingerprints_keep and before dst's next evaluation; the call waits for it.
 * KPE_E_INVALID: a null argument, nsrcs < 1, an unknown bit of what, npairs other than dst's rows, dst
 * among the sources, a pair outside its source or naming a retired row. KPE_E_STATE: dst or a source
 * is not uploaded to dev; a listed source keeps nothing of a requested kind; the kept rule names of
 * the listed sources differ in count, order or text. All checked before any device call. */
#define KPE_GATHER_MATRIX 1u
#define KPE_GATHER_FINGERPRINTS 2u
kpe_status kpe_results_gather(kpe_device* dev, kpe_corpus* dst, const kpe_corpus* const* srcs, int nsrcs,
                              const uint64_t* pairs, uint64_t npairs, uint32_t what);
/* The rows whose fingerprint under the last evaluation of prog differs from the kept one, ascending:
 * the first min(total, cap) row indices into rows[], and, when not NULL, those rows of the new matrix
 * (R bytes each) into verdict_rows[] and their new fingerprints into fps_out[]; memory past that is
 * not written. rows == NULL with cap == 0 counts only. Returns the total, or -kpe_status: KPE_E_INVALID
 * for a null argument, cap > 0 without rows or an unknown flag, KPE_E_LIMIT, then KPE_E_STATE when
 * nothing is kept, the corpus has no evaluation of prog, or masks are asked for and were not written.
 * The kept fingerprints are not modified: call kpe_fingerprints_keep to move on. */
int64_t kpe_changed_rows_fp(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, const uint64_t* salts,
                            const uint64_t* msg_salts, uint8_t msg_codes, uint32_t flags, uint64_t* rows,
                            uint8_t* verdict_rows, uint64_t* fps_out, uint64_t cap);
/* The fingerprint form of kpe_changed_pairs: the fingerprint of row new_row of the last evaluation of
 * prog on c_new under (salts, msg_salts, msg_codes, flags) against c_old's KEPT fingerprint of
 * old_row. Writes the changed pairs' indices, their rows of the new matrix and their new
 * fingerprints (fps_out, may be NULL), with kpe_changed_rows_fp's cap and error conventions;
 * KPE_E_INVALID also for a pair's row outside its corpus, KPE_E_STATE when c_old keeps no
 * fingerprints or either corpus is not uploaded to dev. The host form is kpe_row_fingerprints_host
 * over the gathered rows against kpe_fingerprints_fetch. */
int64_t kpe_changed_pairs_fp(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c_new, const kpe_corpus* c_old,
                             const uint64_t* pairs, uint64_t npairs, const uint64_t* salts, const uint64_t* msg_salts,
                             uint8_t msg_codes, uint32_t flags, uint64_t* changed, uint8_t* verdict_rows,
                             uint64_t* fps_out, uint64_t cap);
/* The host twin of the comparison: the indices i < n with old_fp[i] != new_fp[i], same cap / count-only /
 * return conventions. Host only. */
int64_t kpe_changed_fingerprints_host(const uint64_t* old_fp, const uint64_t* new_fp, uint64_t n, uint64_t* rows,
                                      uint64_t cap);

/* ---- per-namespace rule counts ---------------------------------------------- */
/* The verdict matrix reduced by namespace group on the device: per (group, rule) the cells of each
 * raw verdict code. `fail` counts KPE_FAIL cells whether or not the policy is scored, `warn`
 * KPE_WARN, `undecided` KPE_UNDECIDED; KPE_NA is not counted (kpe_corpus_namespace_rows gives it).
 * The scored / audit fold is the consumer's (kpe_cli_summary_ns): the action depends on the group.
 * It is the table per-namespace compliance views are built from, and what `kyverno apply
 * --audit-warn` needs for policies with validationFailureActionOverrides
 * (ResultCounts.addEngineResponse, cmd/cli/kubectl-kyverno/processor/result.go:53, asks
 * response.GetValidationFailureAction(), a function of the policy, the resource's GetNamespace()
 * and that namespace's labels, engineresponse.go:196-225), without copying the N x R matrix back. */
typedef struct kpe_ns_counts {
  uint32_t pass, fail, warn, error, skip, undecided;
} kpe_ns_counts; /* 24 bytes */
/* Groups [g0, g0 + ng) of the last evaluation of prog on the corpus: out[(g - g0) * R + r]. After
 * kpe_evaluate / kpe_evaluate_async / kpe_evaluate_batch_async of prog on the corpus (waits for it;
 * KPE_E_STATE without one), like kpe_fetch_row_summaries. KPE_E_INVALID when g0 + ng > G or for a
 * null argument (checked before any device call); ng == 0 writes nothing; memory past ng * R
 * entries is not written. KPE_E_LIMIT for 2^32 rows or more (32-bit counters). The first call on an
 * uploaded corpus builds the corpus's rows-by-namespace index and keeps it on the device. */
kpe_status kpe_fetch_namespace_counts(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, uint64_t g0,
                                      uint64_t ng, kpe_ns_counts* out);
/* The same fold over N x R verdict bytes the caller holds (N = the corpus's rows). Host only; no
 * device call. */
kpe_status kpe_namespace_counts_host(const kpe_program* prog, const kpe_corpus* c, const uint8_t* verdicts,
                                     uint64_t g0, uint64_t ng, kpe_ns_counts* out);

/* PSA check id k (bit k of a check mask), e.g. "capabilities_restricted". */
const char* kpe_pss_check_id(int k);
int kpe_pss_num_checks(void);

/* Versioned-check form of the check masks (after kpe_evaluate / kpe_evaluate_async with
 * masks): N x R uint32, bit v = PSA versioned check v failed (0 unless the cell is FAIL).
 * A rule pinned to a version runs every version of a check up to it
 * (pkg/pss/evaluate.go:51-66, evaluatePSS), so one check id can fail more than once;
 * kpe_pss_cv_check(v) is the check id index of versioned check v. Bit 31 (KPE_CVM_XMATCH)
 * of a FAIL cell of a rule with a podSecurity PolicyException: the exception matched the
 * resource, so its exclusions shape the cell's fail message (kpe_report_results_msg). */
#define KPE_CVM_XMATCH (1u << 31)
/* The versioned-check bits of a cv mask word (bits 0 .. kpe_pss_num_cv() - 1): mask with it
 * before walking set bits as versioned checks (bit 31 is a flag, not a check). */
#define KPE_CVM_CHECKS_ALL 0x7FFFFFFFu
kpe_status kpe_fetch_cv_masks(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, uint32_t* cv_masks);
int kpe_pss_num_cv(void);
int kpe_pss_cv_check(int v);

/* `kyverno apply` summary line (cmd/cli/kubectl-kyverno/processor/result.go:34-68) from the
 * per-rule counts of kpe_evaluate / kpe_fetch: unscored fails (policies.kyverno.io/scored:
 * "false") and, with audit_warn (--audit-warn), fails of Audit policies count as warn; a
 * response is counted once per validate rule of its policy with the same name (the
 * reference matches by name). KPE_E_UNSUPPORTED when audit_warn meets
 * validationFailureActionOverrides (the action then depends on each resource's namespace). */
typedef struct kpe_cli_totals {
  uint64_t pass, fail, warn, error, skip;
} kpe_cli_totals;
kpe_status kpe_cli_summary(const kpe_program* prog, const kpe_counts* counts, int audit_warn, kpe_cli_totals* out);
/* The same summary line from the per-namespace table (counts: G x R entries, every group of the
 * corpus), with the action resolved per group: for policies with validationFailureActionOverrides
 * it restates GetValidationFailureAction (engineresponse.go:196-225). Overrides are taken in
 * order; one whose action is not audit / enforce / Audit / Enforce is skipped (api/kyverno/v1/
 * spec_types.go:39-41). With `namespaces` absent (nil) the override applies when CheckSelector
 * (pkg/utils/match/labels.go:10-24) holds for namespaceSelector over the group's namespace labels:
 * a nil selector is false, a selector that does not build is false, wildcards in matchLabels keys
 * and values are expanded against the labels first (wildcards.ReplaceInSelector). Otherwise it
 * applies when an entry of `namespaces` matches the group's name (go-wildcard) and the selector is
 * nil or holds; `namespaces: []` (present, empty) never applies. The first applying override gives
 * the action, else spec.validationFailureAction. The labels are the corpus's namespace label table
 * entry of the group's name (none: empty), as the CLI passes NamespaceSelectorMap[GetNamespace()]
 * (policy_processor.go:63). The fold is kpe_cli_summary's: an unscored fail is a warn; a fail is a
 * warn when audit_warn is set and the resolved action is Audit. Without overrides the totals equal
 * kpe_cli_summary over the per-rule sums. Host only. */
kpe_status kpe_cli_summary_ns(const kpe_program* prog, const kpe_corpus* c, const kpe_ns_counts* counts,
                              int audit_warn, kpe_cli_totals* out);

/* PolicyReport results of one resource (pkg/utils/report/results.go:89-156,
 * EngineResponseToReportResults), as the JSON array encoding/json writes for
 * []PolicyReportResult: one object per rule with a response, in rule order, with
 * source, policy (cache.MetaNamespaceKeyFunc key), rule, result (unscored fail => warn),
 * scored, properties {controls, standard, version} for failing podSecurity rules,
 * category and severity. No message (kpe_report_results_msg / _ex) and no timestamp.
 *   verdict_row : R verdict cells of the resource (kpe_evaluate row)
 *   cv_mask_row : R cells of kpe_fetch_cv_masks, or NULL (then no controls)
 * Writes at most cap-1 bytes plus NUL; returns the full length (call again with a larger
 * buffer when it is >= cap), or a negative kpe_status. Host only; no device call. */
long kpe_report_results(const kpe_program* prog, const uint8_t* verdict_row, const uint32_t* cv_mask_row, char* buf,
                        size_t cap);
/* kpe_report_results with the RuleResponse `message` of each result, rendered from the
 * resource's JSON (the EngineResponse resource, resource_len bytes): podSecurity pass
 * ("Validation rule '<rule>' passed.", validate_pss.go:85) and fail (validate_pss.go:108:
 * FormatChecksPrint of the failing checks after convertChecks; with podSecurity.exclude or a
 * podSecurity PolicyException, over the checks their exclusions leave), validate.pattern pass
 * ("validation rule '<rule>' passed.", validate_resource.go:339), validate.deny pass
 * ("validation rule '<rule>' passed.") and, when the deny block's condition message is known
 * without the resource (no condition `message`, or conditions folded at compile time), fail
 * (getDenyMessage, validate_resource.go:279-300: the rule message joined with the condition
 * message, or "validation error: rule <rule> failed" when both are empty); preconditions skips
 * of deny rules whose preconditions carry no `message` ("preconditions not met", engine.go:283)
 * and of preconditions folded at compile time; a PolicyException skip ("rule skipped due to
 * policy exception <key>") when it is the skip's only cause. A message with variables is
 * substituted over the resource (variables.SubstituteAll, vars.go:311-389) when every variable
 * is a `request.object` path of members and [N] indexes. A substitution error (a member missing
 * from an object) fails SubstituteAll: the pattern message is then not rendered (its reference
 * text embeds the Go error string), and getDenyMessage returns the condition message as is.
 * Messages with other variables are not rendered. Condition messages that depend on where a
 * block stopped need the condition traces (kpe_report_results_ex). Host only. */
long kpe_report_results_msg(const kpe_program* prog, const uint8_t* verdict_row, const uint32_t* cv_mask_row,
                            const char* resource_json, size_t resource_len, char* buf, size_t cap);

/* Failing paths of pattern cells, for their report messages (validate_resource.go:316-454;
 * validate.go MatchPattern PatternError.Path). After kpe_evaluate / kpe_evaluate_async of the
 * same program and corpus, for each listed cell (row * R + column) the device re-walks every root
 * of the cell's validate.pattern / anyPattern rule (at most KPE_TRACE_ROOTS; for a FAIL / ERROR
 * cell of a validate.foreach rule that a pattern entry decided, that entry's roots on the
 * element it validated, kpe_fetch_cond_traces_ex) and records the
 * path of the failure that decided it: out[i * KPE_TRACE_ROOTS * KPE_TRACE_WORDS + k *
 * KPE_TRACE_WORDS + w], w = 0: component count (bits 0-7) | KPE_TR_TRUNC | the root's verdict
 * << 16 | KPE_TR_VALID; w = 1..15: components (a pattern member, KPE_TC_KEY | key id, or
 * KPE_TC_IDX | array index). A cell of a rule without patterns gives a zero record. */
#define KPE_TRACE_WORDS 16u
#define KPE_TRACE_ROOTS 4u
#define KPE_TC_IDX 0x80000000u
#define KPE_TC_KEY 0x40000000u
#define KPE_TR_TRUNC 0x100u
#define KPE_TR_VALID 0x1000000u
kpe_status kpe_pattern_traces(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, const uint64_t* cells,
                              uint64_t ncells, uint32_t* out);
/* kpe_report_results_msg plus the pattern messages: `traces` holds the row's R cells in
 * kpe_pattern_traces layout (R * KPE_TRACE_ROOTS * KPE_TRACE_WORDS words; only pattern-rule
 * cells are read). Adds: validate.pattern fail ("validation error: <message>. rule <rule> failed
 * at path <path>", buildErrorMessage), anyPattern pass ("validation rule '<rule>' anyPattern[<i>]
 * passed.") and fail (buildAnyPatternErrorMessage over "rule <rule>[<i>] failed at path <path>").
 * The rule message is substituted as in kpe_report_results_msg. Not rendered (no message):
 * messages with other variables or a failed substitution, empty-path failures (their text is the
 * Go error string), skips, anyPattern fails with more than KPE_TRACE_ROOTS patterns. */
long kpe_report_results_msg_tr(const kpe_program* prog, const kpe_corpus* corpus, const uint8_t* verdict_row,
                               const uint32_t* cv_mask_row, const uint32_t* traces, const char* resource_json,
                               size_t resource_len, char* buf, size_t cap);

/* Condition traces, for the condition messages of validate rules (variables/evaluate.go:31-125):
 * after kpe_evaluate / kpe_evaluate_async of the same program and corpus, rows [row0, row0 +
 * nrows) into out (nrows x R words, row-major). A rule whose preconditions are evaluated per
 * resource, or whose validate.deny conditions carry a `message`, records where each block
 * stopped: the preconditions in bits 0-15, the deny block in bits 16-31, each as the index of
 * the first true `any` condition (bits 0-6), of the first false `all` condition (bits 7-13),
 * 0x4000 evaluated without an error, 0x8000 it held. Other cells (and blocks of more than 127
 * conditions) are 0. */
kpe_status kpe_fetch_cond_traces(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, uint64_t row0,
                                 uint64_t nrows, uint32_t* out);
/* Condition traces with the foreach and error records (report time): rows [row0, row0 + nrows)
 * into out, nrows x R x KPE_CTRACE_WORDS words. Word 0 of a cell is kpe_fetch_cond_traces' word,
 * where a block that raised an error records which condition raised it and on which side
 * (KPE_CT_ERR without the evaluated bit 0x4000: bits 0-6 the condition, any conditions first,
 * then all; bits 7-8 0 the key's substitution, 1 the value's, 2 the operator). For validate.foreach
 * rules (validateElements, validate_resource.go:206-254) the words describe the element that
 * decided a FAIL / ERROR cell: word 0 bits 16-31 its deny block (or its preconditions' error),
 * word 1 its path (nesting depth, what decided it, per level the entry and the element index),
 * words 2 and 3 the element's and the validated element's document nodes. The words of other cells
 * and of foreach cells that are not FAIL / ERROR are unspecified. */
#define KPE_CTRACE_WORDS 4u
#define KPE_CT_ERR 0x8000u
kpe_status kpe_fetch_cond_traces_ex(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, uint64_t row0,
                                    uint64_t nrows, uint32_t* out);
/* kpe_report_results_msg_tr plus the condition messages of kpe_fetch_cond_traces (cond_traces:
 * the row's R words, or NULL) or kpe_fetch_cond_traces_ex (cond_traces_ex, the row's R x
 * KPE_CTRACE_WORDS words; it takes precedence):
 *   - a preconditions skip (engine.go:282-284): "preconditions not met; <condition message>" of
 *     any validate rule, for preconditions evaluated per resource or folded at compile time;
 *   - validate.deny fail: getDenyMessage (validate_resource.go:279-300), the rule message joined
 *     with the deny block's condition message by "; " and substituted over the resource (on a
 *     substitution error the condition message as is);
 *   - a PolicyException skip of a rule whose preconditions read the resource, once the trace
 *     shows they held ("rule skipped due to policy exception <key>").
 * Preconditions and deny conditions are not substituted into condition messages before they join
 * (the reference substitutes only getDenyMessage's joined text).
 * With cond_traces_ex (and the corpus, for the element's document):
 *   - validate.foreach pass: "rule passed" (validate_resource.go:203); fail / error: the deciding
 *     element's response wrapped once per nesting level, "validation failure: <message>"
 *     (:239-247), where <message> is getDenyMessage over the element's context, the pattern /
 *     anyPattern message of the entry's walk on the element (kpe_pattern_traces records the
 *     foreach cell's element walk), or a RuleError text below; AddElementToContext's
 *     "failed to process foreach: cannot use elementScope=true ..." (:218-221);
 *   - RuleError texts: "failed to evaluate preconditions: <err>" (engine.go:279-281,
 *     validate_resource.go:125-128), "failed to check deny conditions: <err>" (:269-271),
 *     "variable substitution failed: <err>" (:139-141), "failed to deserialize anyPattern, expected
 *     type array: <err>" (:347-350), with <err> the substitution error the reference words itself:
 *     "failed to substitute variables in condition key|value: failed to resolve <var> at path <path>:
 *     JMESPath query failed: Unknown key \"<k>\" in path" (variables/evaluate.go:14-27, vars.go:
 *     311-389, context/evaluate.go:27-31), "invalid query (nil)", "expected string after
 *     substituting variables in key ...", "failed to create handler for condition operator".
 * Not rendered: pattern skips and empty-path pattern errors (their text is validate.go's chain of
 * anchor errors with Go %v renderings of resource and pattern values), errors whose text
 * go-jmespath words itself (a function's argument error), messages with variables outside the
 * restated paths, element<n> variables of an outer foreach level, and the RuleResponse timestamp. */
typedef struct kpe_report_args {
  const kpe_program* prog;
  const kpe_corpus* corpus;        /* pattern traces' key names; may be NULL without pattern traces */
  const uint8_t* verdict_row;      /* R verdict cells */
  const uint32_t* cv_mask_row;     /* R cells of kpe_fetch_cv_masks, or NULL */
  const uint32_t* pattern_traces;  /* kpe_pattern_traces layout for the row, or NULL */
  const uint32_t* cond_traces;     /* R words of kpe_fetch_cond_traces, or NULL */
  const char* resource_json;       /* the resource (NULL: no messages) */
  size_t resource_len;
  const uint32_t* cond_traces_ex;  /* R x KPE_CTRACE_WORDS words of kpe_fetch_cond_traces_ex, or NULL */
} kpe_report_args;
long kpe_report_results_ex(const kpe_report_args* args, char* buf, size_t cap);

/* ---- reports for a row list -------------------------------------------------- */
/* The last step of the delta pipeline (kpe_changed_rows / kpe_changed_rows_fp give the rows whose
 * report changes): for a list of rows the device selects the cells whose report entry needs detail
 * and gathers it, one call brings it back in sparse form, and one host call renders every listed
 * report. The per-row calls above are the specification: the bulk path reproduces them byte for byte.
 *
 * Which cells need which detail, per rule, in the KPE_SEL convention of kpe_select_cells (R bytes
 * each): cell (row, r) with verdict v needs the kind iff (sel[r] >> v) & 1.
 *   mask_sel    : the check mask word: a KPE_FAIL cell of a podSecurity rule; 0 for other rules;
 *   cond_sel    : the condition trace words: a KPE_FAIL / KPE_ERROR / KPE_SKIP cell of a rule with a
 *                 condition trace slot; 0 for a rule without one;
 *   pattern_sel : the pattern record: a KPE_FAIL cell of a validate.pattern / anyPattern rule, a
 *                 KPE_PASS cell of an anyPattern rule, a KPE_FAIL / KPE_ERROR cell of a validate.foreach
 *                 rule with a pattern entry; 0 for a rule without a pattern walk.
 * KPE_NA and KPE_UNDECIDED are never selected. Host only. */
kpe_status kpe_report_detail_need(const kpe_program* prog, uint8_t* mask_sel, uint8_t* cond_sel, uint8_t* pattern_sel);

#define KPE_RR_MASKS 1u
#define KPE_RR_COND 2u
#define KPE_RR_PATTERNS 4u
/* Three sparse lists over the listed rows. A cell is named k * R + r, k the position in rows[] (not
 * the row id), so the lists are self-contained for the renderer. Each list is ascending in that
 * index and holds the first min(total, cap) entries; nothing past that is written. A cap of 0 with
 * null pointers counts only. The totals are always written.
 *   mask_words     : per cell exactly the word kpe_fetch_cv_masks returns for it (KPE_CVM_XMATCH
 *                    included);
 *   cond_words     : per cell exactly the KPE_CTRACE_WORDS words kpe_fetch_cond_traces_ex returns
 *                    for it (words the rule's slot does not have are zero);
 *   pattern_traces : per cell exactly the record kpe_pattern_traces returns for the absolute cell
 *                    rows[k] * R + r, the element walk of a foreach cell included;
 *   verdict_rows   : when not NULL, the nrows x R verdict cells of the listed rows. */
typedef struct kpe_report_rows {
  uint8_t* verdict_rows;                               /* nrows x R, or NULL */
  uint64_t* mask_cells;    uint32_t* mask_words;       uint64_t mask_cap;    /* 1 word per cell */
  uint64_t* cond_cells;    uint32_t* cond_words;       uint64_t cond_cap;    /* KPE_CTRACE_WORDS per cell */
  uint64_t* pattern_cells; uint32_t* pattern_traces;   uint64_t pattern_cap; /* KPE_TRACE_ROOTS*KPE_TRACE_WORDS per cell */
  uint64_t mask_total, cond_total, pattern_total;      /* out */
} kpe_report_rows;
/* After an evaluation of prog on the corpus, under the state rules of kpe_fetch_row_summaries (waits
 * for it). rows[]: any order, duplicates allowed, every entry < N. flags: the kinds to gather; a kind
 * whose flag is not set gives total 0 and its arrays are not read. KPE_E_INVALID for a null argument,
 * an unknown flag, a cap without its arrays or a row past N, all checked before any device call;
 * KPE_E_STATE without an evaluation of prog, or for KPE_RR_MASKS after an evaluation without masks (as
 * kpe_fetch_cv_masks). No rule limit. The scratch belongs to the device handle and is kept between
 * calls. */
kpe_status kpe_fetch_report_rows(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, const uint64_t* rows,
                                 uint64_t nrows, uint32_t flags, kpe_report_rows* io);
/* The specification twin of the selection, a plain double loop over dense inputs the caller holds for
 * the listed rows: nrows x R verdicts, nrows x R mask words (may be NULL without KPE_RR_MASKS) and
 * nrows x R x KPE_CTRACE_WORDS trace words (may be NULL without KPE_RR_COND). Same lists, caps and
 * totals; of the pattern kind only pattern_cells is written (there are no records without a device)
 * and verdict_rows is not touched. Host only. */
kpe_status kpe_report_cells_host(const kpe_program* prog, uint64_t nrows, const uint8_t* verdict_rows,
                                 const uint32_t* cv_mask_rows, const uint32_t* cond_ex_rows, uint32_t flags,
                                 kpe_report_rows* io);
/* The bulk renderer: `in` carries verdict_rows, the three lists and their entry counts in the *_total
 * fields (fewer entries than the device total is legal when a list was truncated; null lists are
 * legal). Row k's JSON array is buf[offsets[k] .. offsets[k+1]), with no separators; offsets has
 * nrows + 1 entries and is always written. resources[k] (resource_lens[k] bytes) may be NULL: then
 * row k gets no messages, as kpe_report_results gives. Returns the total length; when it is >= cap
 * nothing useful is in buf and the caller calls again, as with kpe_report_results; a negative return
 * is -kpe_status. For every row the bytes equal kpe_report_results_ex over the row's dense inputs,
 * where an input is NULL when the row has no entry in that list (so the rows past the cut of a
 * truncated list render without that detail). Rows are rendered on up to 16 threads
 * (KPE_REPORT_THREADS lowers it); the output does not depend on the thread count. Host only; no
 * device call. */
long kpe_report_results_rows(const kpe_program* prog, const kpe_corpus* corpus, uint64_t nrows,
                             const kpe_report_rows* in, const char* const* resources, const size_t* resource_lens,
                             char* buf, size_t cap, uint64_t* offsets /* nrows + 1 */);

/* ---- instrumentation (HIP events on the evaluation stream) ---------------- */
typedef struct kpe_kernel_stats {
  uint64_t launches;        /* timed launches since the last reset: one per evaluation, one per
                               multi-shard LEAN launch of kpe_evaluate_batch_async */
  double pss_kernel_ms;     /* summed duration of the resource-scan kernel      */
  double dict_kernel_ms;    /* summed duration of the dictionary predicate pass */
  double scan_bytes;        /* algorithmic bytes one scan-kernel launch reads+writes */
  double pattern_kernel_ms; /* summed duration of the kernels after the scan (condition, exclusion,
                               pattern-rule kernels; 0 without such rules) */
  double pattern_bytes;     /* algorithmic bytes of one pattern-kernel launch: every resource's
                               document tape (8 B per entry) and root offset once, plus the verdict
                               matrix read and written */
  int32_t scan_kernel;      /* the scan instantiation of the last timed launch: 1 kpe_scan_kernel
                               (general), 2 its LEAN instantiation (corpora past 4 GiB of pod
                               records), 7 kpe_lean6_kernel (one shard), 9 kpe_lean6_kernel (a multi-shard launch) */
  int32_t pad_;
  double scan_bytes_sum;    /* algorithmic bytes of every timed scan-kernel launch since the last reset,
                               summed (multi-shard launches differ in size: the mean launch carries
                               scan_bytes_sum / launches, not the last launch's scan_bytes) */
  double pattern_bytes_sum; /* the same for the pattern kernel's algorithmic bytes */
  double pss_kernel_ms_min, pss_kernel_ms_max, pss_kernel_ms_sq;  /* the scan launches' shortest and
                               longest duration and the sum of squared durations (spread) */
} kpe_kernel_stats;
kpe_status kpe_device_set_timing(kpe_device* dev, int enabled);
kpe_status kpe_device_kernel_stats(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c,
                                   kpe_kernel_stats* out, int reset);

#ifdef __cplusplus
}
#endif
#endif /* KPE_H_ */
