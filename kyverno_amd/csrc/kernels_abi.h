// Kernel argument structs shared by the kernel sources (*.hip, device) and kpe_api.cpp (host). No HIP
// types here (the host check programs under scripts/ include it); the launchers are declared in
// kernels_launch.h.
#pragma once
#include <stdint.h>

#include "schema.h"

#define PRED_LOCAL 0x80000000u  // pred_word flag: bitset lives in the scan block's LDS

// ScanArgs.need: which columns / lists the compiled program reads
#define NEED_FLAGS (1u << 0)
#define NEED_GVK (1u << 1)
#define NEED_CAPS (1u << 2)
#define NEED_SANN (1u << 3)
#define NEED_VOL (1u << 4)
#define NEED_SYS (1u << 5)
#define NEED_PANN (1u << 6)
#define NEED_NSA (1u << 7)
#define NEED_LAB (1u << 8)   // resource labels (CSR) for label selectors
#define NEED_NSL (1u << 9)   // namespace label table for namespaceSelector
#define NEED_NAME (1u << 10) // r_name (name / names terms)
#define NEED_MNS (1u << 11)  // r_mns (namespaces terms)

// Pattern classes (host-classified go-wildcard patterns; '?' or an inner '*' => PK_GLOB)
#define PK_ANY 0u       // "*"
#define PK_EXACT 1u     // no wildcard
#define PK_PREFIX 2u    // "lit*"
#define PK_SUFFIX 3u    // "*lit"
#define PK_CONTAINS 4u  // "*lit*"
#define PK_GLOB 5u      // general: full pattern text
#define PK_QNAME 6u     // validation.IsQualifiedName (apimachinery v0.29.1, label keys)
#define PK_LABVAL 7u    // validation.IsValidLabelValue
#define PK_NONEMPTY 8u  // '*'s around one '?' ("?*", "*?", "*?*"): one rune or more, i.e. non-empty
struct KpePat {
  uint32_t kind, off, len, pad;  // literal (or full pattern for PK_GLOB) = pat_bytes[off, off+len)
};

// One work item of the per-namespace count kernels (kpe_launch_ns_counts, results.hip): rows
// [begin, end) of the corpus's rows-by-namespace list, all of namespace group g, at most
// kpe_ns_chunk_rows() of them. single: the group's only item (its counters are stored, not added).
struct KpeNsItem {
  uint32_t g, begin, end, single;
};

// Report detail of a row list (kpe_launch_report_need_scatter, report_rows.inl). Src: rows[] (every
// entry a row of the corpus), the N x R check mask words (read only for mask hits), the N x nmsg
// condition trace words and the per-rule slot table (KPE_RR_SLOT; both read only for cond hits).
// Out: per kind the list of compact cells and its payload, written below the kind's cap only;
// pattern_abs holds the absolute cell rows[i] * R + r, the list kpe_launch_pattern_trace takes.
// slot table entry of a rule: its first word in a row's nmsg condition trace words << 3 | how many
// words it has (0: no slot, 1, or KPE_FE_TRACE_WORDS for a validate.foreach rule)
#define KPE_RR_SLOT(first, width) (((uint32_t)(first) << 3) | (uint32_t)(width))
#define KPE_RR_SLOT_FIRST(e) ((e) >> 3)
#define KPE_RR_SLOT_WIDTH(e) ((e) & 7u)
struct KpeRrSrc {
  const uint64_t* rows;
  const uint32_t* masks;
  const uint32_t* mtrace;
  const uint32_t* slot;
  uint32_t nmsg, pad_;
};
struct KpeRrOut {
  uint64_t* mask_cells;
  uint32_t* mask_words;  // 1 per cell
  uint64_t mask_cap;
  uint64_t* cond_cells;
  uint32_t* cond_words;  // 4 per cell
  uint64_t cond_cap;
  uint64_t* pattern_cells;
  uint64_t* pattern_abs;
  uint64_t pattern_cap;
};

struct PredJob {
  uint32_t domain;
  uint32_t pat0, npat;  // patterns [pat0, pat0+npat) of the pattern table
  uint32_t out_word;    // first output word
  uint32_t blk0;        // first block of this job
};

struct PredArgs {
  const uint8_t* dict_bytes[KPE_NUM_DOMAINS];
  const uint32_t* dict_off[KPE_NUM_DOMAINS];
  uint32_t dict_n[KPE_NUM_DOMAINS];
  const uint8_t* pat_bytes;
  uint32_t pat_len;
  const KpePat* pats;  // pattern records
  const PredJob* jobs;
  uint32_t njobs;
  uint32_t* out;
};


// Predicate references in the scan kernel's tables are resolved per binding to
// bitset locations: PRED_LOCAL | LDS word index, or a pbuf word index; PRED_NONE = absent.
#define PRED_NONE 0xFFFFFFFFu
#define KPE_RULE_CHUNK 32  // rules evaluated per transposed pass (one rule per lane)

// Rule lane record (uint4, one per rule, evaluated by one lane in the transposed pass):
//   x = handler | cv_class << 4 | match_mode << 16 | excl_mode << 18
//   y = match_f0 | match_nf << 24, z = excl_f0 | excl_nf << 24, w = pol_term (PRED_NONE: none)
#define RL_HANDLER(x) ((x) & 0xFu)
#define RL_CV(x) (((x) >> 4) & 0xFFFu)
#define RL_MATCH_MODE(x) (((x) >> 16) & 3u)
#define RL_EXCL_MODE(x) (((x) >> 18) & 3u)
#define RL_F0(y) ((y) & 0xFFFFFFu)
#define RL_NF(y) ((y) >> 24)

// NARROW programs (<= KPE_NARROW_TERMS distinct terms, <= KPE_NARROW_R rules): each
// lane evaluates every rule for its own resource from a term bit vector.
// Narrow rule record (uint4): x = handler | match_mode << 4 | excl_mode << 6 |
//   NR_APPLY_ONE | NR_NEW_POLICY | (pol_term + 1) << 16 (0: no namespaced-policy term),
//   y = cv_mask, z = match filters (RL_F0 / RL_NF), w = exclude filters;
//   fmask[f] = bit mask of the terms filter f ANDs.
#define KPE_NARROW_TERMS 32
#define KPE_NARROW_R 32
#define KPE_NARROW_FILTERS 64
#define KPE_TT_TERMS 8
#define NR_HANDLER(x) ((x) & 0xFu)
#define NR_MATCH_MODE(x) (((x) >> 4) & 3u)
#define NR_EXCL_MODE(x) (((x) >> 6) & 3u)
#define NR_APPLY_ONE (1u << 8)
#define NR_NEW_POLICY (1u << 9)
#define NR_POLTERM(x) ((x) >> 16)

// Per-wave PSS list staging (LDS): 128 container entries (uint2), 128 one-byte volume codes,
// 64 one-byte codes each for sysctls and pod annotations.
#define KPE_STAGE_CTR 128
#define KPE_STAGE_VOL 128  // pods average > 1 volume (C2: 1.4): two preloaded slots per lane
#define KPE_STAGE_SMALL 64
#define KPE_STAGE_WORDS ((KPE_STAGE_CTR * 8 + KPE_STAGE_VOL + 2 * KPE_STAGE_SMALL) / 4)

struct ScanArgs {
  int64_t n;
  // resource rows (unstructured view) — read by match terms
  const uint32_t *r_gvk, *r_name, *r_mns, *r_nsa, *ann_off, *ann_k, *ann_v;
  const uint32_t *lab_off, *lab_k, *lab_v;           // metadata.labels CSR
  const uint32_t *r_nsl, *nsl_off, *nsl_k, *nsl_v;   // namespace label table row per resource
  // PSS hot records (schema.h): pod records, wave headers, container records
  const uint32_t* rec;        // 4 words per pod
  const uint32_t* hdr;        // 4 words per 64 pods
  const uint32_t* crec;       // 2 words per container
  const uint32_t* vol_src;    // per volume: VolumeSource presence mask
  const uint32_t* sys_id;     // per sysctl: D_SYSCTL id
  const uint32_t* pann_kv;    // per pod-template annotation: (D_ANNK id, D_ANNV id)
  const uint32_t* c_sann;     // per container: value id of its seccomp annotation (cold)
  uint32_t ntiles;            // ceil(n / 64); hdr has ntiles + 1 entries
  const uint32_t* zero_page;  // >= 64 zero bytes: source of the loads of unneeded columns
  const uint32_t* capsets;    // capability-set dictionary: 4 words (add lo/hi, drop lo/hi) per set
  uint32_t ncapsets;
  uint32_t nctr_total, nvol_total, nsys_total, npann_total;  // list lengths (load clamping)
  // program tables; predicate fields resolved to bitset locations (binding copies)
  const KpeRule* rules;
  const uint32_t* rule_lanes;  // packed rule lane records (RL_*)
  const uint32_t* narrow_rules;  // NARROW: 4 words per rule (NR_*)
  const uint32_t* rule_exc;      // KpeRule::exc per rule (XE_*), or null: no PolicyExceptions
  const uint32_t* fmask;         // NARROW: term mask per filter
  uint32_t nfilters;
  // NARROW truth-table fast path (tt_lds != PRED_NONE: <= KPE_TT_TERMS terms, no ApplyOne):
  // every block tabulates matched-rule masks for all 2^nterms term vectors in LDS at
  // tt_lds; narrow_cls holds (cv_mask, rule mask) per distinct PSS version set.
  uint32_t tt_lds, ncls, pss_rules, err_rules, pat_rules;
  const uint32_t* narrow_cls;
  const KpeFilter* filters;
  const uint32_t* fterms;
  const KpeTerm* terms;
  const KpeKindSel* kindsels;
  const KpeAnnPair* annpairs;
  const KpeSelector* selectors;
  const KpeSelReq* selreqs;
  const uint32_t* cv_classes;  // distinct PSS cv_masks (rule.cv_class indexes them)
  uint32_t filt_lds, fterm_lds, nfterms;  // filters / filter terms staged in LDS at these word
                                          // offsets (filt_lds == PRED_NONE: read from HBM)
  uint32_t nrules, nterms, ncv, any_apply_one;
  // predicate bitsets: pbuf[0, blob_words) = small-domain bitsets, copied into LDS by
  // every block (same word indices); the rest = large-domain bitsets (HBM/L2)
  const uint32_t* pbuf;
  uint32_t blob_words;
  // Fused dictionary pass (npairs > 0): every block evaluates the small-domain
  // predicates itself from the binding's fuse image, copied into LDS at fuse_lds:
  // [pair table (uint2 per (string, pattern))][KpePat table][pattern bytes][strings].
  // Pair: x = string LDS byte address | length << 20; y = pattern index |
  // bitset word << 12 | bit << 27 (OR-ed in with an LDS atomic).
  const uint32_t* fuse;
  uint32_t fuse_words, fuse_lds, npairs;
  uint32_t fuse_pats, fuse_patb;  // LDS word index of the pattern table / pattern bytes
  uint32_t wave_lds, wave_words;  // per-wave LDS regions: dyn[wave_lds + wv * wave_words ...]
  // fixed PSS predicates (resolved locations)
  uint32_t pp_apparmor_key, pp_apparmor_ok, pp_seccomp_pod_key, pp_seccomp_ann_ok;
  uint32_t pp_caps_ok, pp_cap_nbs, pp_cap_all, pp_sysctl0, pp_sysctl1, pp_sysctl2;
  uint32_t cv_union, need;
  // Prologue image (kpe_scan_kernel<..., PREP = true>, one block per binding, writes it): a
  // copy of the scan block's LDS words [0, pimg_words) = [predicate bitsets (blob_words)]
  // [truth table at tt_lds][kind table at kt_lds][capability-set bits (bytes) at capb_lds].
  // Every scan block copies it into LDS with straight 16-byte loads. Null: every scan block
  // computes its own prologue (the fuse area then sits at fuse_lds, after the wave regions).
  uint32_t* pimg;
  uint32_t pimg_words, capb_lds;
  // LEAN scans (kind-only match terms): kt[kind id] = matched-rule mask (PRED_NONE: no table)
  uint32_t kt_lds, nkinds;
  const uint32_t* psum;  // PSUM general scan: per-pod scan records (3 words per pod: pod word, failing versioned checks, kind << 16)
  // Selector requirement masks (selm bit 0: label selectors, bit 1: namespaceSelectors; built
  // per binding by kpe_selmask_kernel). Requirement q of a selector is bit qbit + q. Label
  // selectors: sel_km[key id] = {requirements whose key glob holds, wildcard requirements whose
  // key is a valid qualified name} and sel_vm[value id] = {requirements whose value set holds,
  // wildcard requirements whose value is a valid label value}, 64-bit each, folded per row over
  // its labels in order; sm_* = the requirements of each operator class. namespaceSelectors:
  // ns_q[namespace row] = the requirements that hold on that namespace's labels (row ns_none:
  // a resource without a namespace row).
  const uint4* sel_km;
  const uint4* sel_vm;
  const uint64_t* ns_q;
  uint32_t selm, ns_none, nlabk, nlabv;
  // sel_km then sel_vm staged in each scan block's LDS at this word offset (the label fold then
  // reads LDS, not L2), or PRED_NONE
  uint32_t selt_lds, selt_pad;
  // kind terms (T_KSLOT): LDS word offset of the corpus's distinct GVKs (ascending, nkslot_g of
  // them, padded to an even count) followed by each one's 64-bit kind-term mask; PRED_NONE: none
  uint32_t kslot_lds, nkslot_g;
  const uint32_t* kslot_tab;  // the table in HBM (copied by every scan block)
  uint64_t sm_pos, sm_wild, sm_notin, sm_exists, sm_dne;
  // outputs
  uint8_t* verdicts;  // n x nrules
  uint32_t* masks;    // n x nrules failing versioned checks (bit v = KpeCheckVersion v) or null
};

// The PSA dictionary codes of a corpus (lean.inl kpe_psa_codes_kernel): the four dictionaries it
// codes (PsaCodeArgs::dict_*[PSD_*]) and the fixed sets of the PSA library (pss_fixed.hpp) as bits
// of a string's set-hit word (the fixed table's set numbers).
#define PSD_CAP 0
#define PSD_SYSCTL 1
#define PSD_ANNK 2
#define PSD_ANNV 3
#define PSF_CAPS_OK 0
#define PSF_CAP_NBS 1
#define PSF_CAP_ALL 2
#define PSF_SYSCTL0 3
#define PSF_SYSCTL1 4
#define PSF_SYSCTL2 5
#define PSF_APPARMOR_KEY 6
#define PSF_SECCOMP_POD_KEY 7
#define PSF_APPARMOR_OK 8
#define PSF_SECCOMP_ANN_OK 9
// Fixed-set table (psa_fixed_table in kpe_api.cpp), 32-bit words:
//   [0] exact entries E, [1] prefix entries X, [2 + len] (first | end << 16) of the exact entries
//   of byte length len < KPE_PSF_MAXLEN (sorted by length), then E + X entries of 2 words
//   {set | prefix << 7 | len << 8, word index of the literal}, then the literals (4-byte padded).
// A prefix entry is a literal followed by one trailing '*' (go-wildcard: a byte-prefix match).
#define KPE_PSF_MAXLEN 64u
#define KPE_PSF_ENT0 (2u + KPE_PSF_MAXLEN)
// Code bytes of a corpus: [capability sets | sysctls | annotation keys | annotation values], each
// part 4-byte aligned (PsaCodes offsets). Capability set: CS_* bits (scan.hip) | 8: the set
// holds a capability id >= 64 (never read: such a resource is a per-resource limit row); sysctl:
// bit v = outside version v's allowed set; annotation key: bit 0 AppArmor container key, bit 1
// pod seccomp key; annotation value: bit 0 allowed AppArmor profile, bit 1 allowed seccomp profile.
struct PsaCodes {
  uint32_t ncapsets, nsysd, nannk, nannv;  // entries of each part
  uint32_t o_sys, o_annk, o_annv, bytes;   // byte offsets of the parts, total bytes
};
struct PsaCodeArgs {
  const uint8_t* dict_bytes[4];
  const uint32_t* dict_off[4];
  uint32_t dict_n[4];
  const uint32_t* capsets;  // (add lo, add hi, drop lo, drop hi) capability-id masks per set
  const uint32_t* fixed;    // fixed-set table (above)
  uint32_t fixed_words, pad_;
  PsaCodes L;
  uint8_t* codes;           // out
};
// kpe_psum_kernel (the general scan's per-pod PSA records, rebuilt by every evaluation of a
// podSecurity program that is not LEAN, and kpe_corpus_psa_summary)
struct PsumArgs {
  int64_t n;
  uint32_t ntiles, pad_;
  const uint32_t *rec, *hdr, *crec, *vol_src, *sys_id, *pann_kv, *c_sann;
  const uint8_t* codes;  // PsaCodeArgs::codes
  PsaCodes L;
  uint32_t* psum;        // out: 3 words per pod (pod word, failing versioned checks, kind << 16)
  uint32_t* summ;        // out (or null): 2 words per pod (OR of container states, codes; schema.h PS_*)
};

// kpe_selmask_kernel: the selector requirement masks of a binding (ScanArgs::sel_km / sel_vm /
// ns_q) from the predicate bitsets (prologue image for local ones, pbuf for the rest).
struct SelMaskArgs {
  const uint32_t* pimg;      // prologue image: local bitsets at their LDS word index
  const uint32_t* pbuf;      // global bitsets
  const KpeSelReq* reqs;     // resolved requirement records (binding copy)
  const uint32_t* rq;        // label-selector requirement of bit b (selreqs index), nrq entries
  const uint32_t* nq;        // namespaceSelector requirement of bit b, nnq entries
  uint32_t nrq, nnq, nlabk, nlabv, nrows;  // nrows: namespace label table rows (ns_q has nrows + 1)
  uint32_t pad_;
  const uint32_t *nsl_off, *nsl_k, *nsl_v;
  uint4* km;                 // out: nlabk entries
  uint4* vm;                 // out: nlabv entries
  uint64_t* nsq;             // out: nrows + 1 entries
};

// kpe_lean6_kernel: the LEAN evaluation of one or more bound shards of one program in one launch
// (kpe_evaluate_async: one shard; kpe_evaluate_batch_async: up to KPE_LEAN_BATCH). Passed by
// value (< 4 KiB of kernel arguments): block b of the grid belongs to the shard s with
// blk0[s] <= b < blk0[s + 1]. Every launch reads each pod's record and its container, volume,
// sysctl and annotation lists: nothing per pod is carried over from an earlier evaluation.
#define KPE_LEAN_BATCH 24
struct LeanShard {
  const uint32_t *rec, *hdr, *crec, *vol, *sys, *pann, *sann;  // the corpus's PSS columns
  // its compact columns (below): 12-byte pod records; container words, or in a scatter launch
  // the base of the owner-tagged columns (kpe_l6_tag_layout). In a narrow scatter launch rec12
  // is the pod word column pw4 (below; the struct has no room for a pointer more: 4 KiB)
  const uint32_t *rec12, *cw4;
  const uint8_t* codes;  // the corpus's PSA dictionary codes (PsaCodeArgs::codes)
  const uint32_t* kt;     // the binding's kind table: matched-rule mask per kind id (prologue image)
  uint8_t* verdicts;      // n x R
  uint32_t* masks;        // n x R failing versioned checks, or null
  uint32_t n, nkinds, nctr, nvol, nsys, npann;
  PsaCodes L;
};
struct LeanBatchArgs {
  uint32_t nshards, nrules, ncls, cv_union, pss_rules, err_rules, pat_rules, need;
  uint32_t kt_words, code_words, wave_words, tpw;  // LDS: kind table, codes (LC), per-wave stage
  const uint32_t* narrow_cls;  // (cv classes, rule mask) pairs of the program
  // the first KPE_L6_CLS version classes as evidence masks (below; zero past ncls): a pod fails
  // class c when its evidence word meets ev[c], or ev_nw[c] on a pod that is not a Windows pod
  uint32_t cls_ev[4], cls_ev_nw[4], cls_rm[4];
  // kpe_l6_pod_table_word(0 .. KPE_L6_PT_WORDS - 1), one copy per device; a launch that reads the
  // compact columns gets the table and the class masks above in the packed numbering (kpe_l6_pack_ev)
  const uint32_t* pod_tab;
  uint32_t blk0[KPE_LEAN_BATCH + 1];  // a block covers 4 * tpw tiles of 64 pods
  LeanShard sh[KPE_LEAN_BATCH];
};
static_assert(sizeof(LeanBatchArgs) < 4096, "LeanBatchArgs is passed by value: under 4 KiB of kernel arguments");
// Per-wave LDS stage of kpe_lean6_kernel: a tile's staged list items (one word per container,
// volume / sysctl / annotation codes as bytes); items past these counts are loaded again.
#define KPE_L6_CTR 128u
#define KPE_L6_VOL 128u
#define KPE_L6_SMALL 64u
#define KPE_L6_STAGE_BYTES (KPE_L6_CTR * 4u + KPE_L6_VOL + 2u * KPE_L6_SMALL)
// A pod ORs its first four containers with four dword reads from its first slot on: the reads of
// a pod whose containers end at slot KPE_L6_CTR - 1 reach 12 bytes into the volume bytes that
// follow (read, never selected: a word past the pod's count is dropped).
// A staged container: the state bits the PSA checks read (CX_*, in place) with the container's
// codes in bits those leave free: its capability-set code (CS_* of scan.hip) and whether its
// seccomp annotation is outside the allowed profiles. The word of an empty slot is 0.
#define KPE_L6_CX_USED                                                                                          \
  (CX_PRIV_T | CX_APE_T | CX_APE_U | CX_RNR_F | CX_RNR_U | CX_RAU_Z | CX_SEC_NONE | CX_SEC_UNC | CX_SEC_OTHER | \
   CX_PM_OTHER | CX_SEL_OTHER | CX_SEL_USER | CX_SEL_ROLE | CX_WHP_T | CX_HOSTPORT)
#define KPE_L6_CAP_SH 26   // 3 bits (CX_WHP_NT, CX_CAPS, CX_NOCAPS are not read)
#define KPE_L6_SANN_SH 30  // 1 bit (CX_NOHOSTPORT)
// The evidence word of a pod (verdict-only evaluations): the OR of its staged containers, with the
// pod-level fields folded into the container bits they are alternatives of (a pod-level
// runAsUser: 0 sets CX_RAU_Z, a valid pod seccomp type clears CX_SEC_NONE, ...), and the pod's
// list codes and host namespaces in further free bits. Every versioned check is then "some bit
// of kpe_l6_evidence(cv) is set", so a version class fails when the word meets the OR of its
// checks' masks.
#define KPE_L6_CLS 4u
#define KPE_L6_EV_SYS0 (1u << 1)   // sysctl outside the 1.0 / 1.27 / 1.29 sets: bits 1, 2, 4
#define KPE_L6_EV_SYS1 (1u << 2)
#define KPE_L6_EV_SYS2 (1u << 4)
#define KPE_L6_EV_HOSTNS (1u << 6)
#define KPE_L6_VOL_SH 13           // volume code: bit 0 hostPath, bit 1 outside the restricted set
#define KPE_L6_ANN_SH 17           // annotation code: bit 0 AppArmor, bit 1 pod seccomp annotation
#if defined(__HIPCC__)
#define KPE_L6_FN __host__ __device__ inline
#define KPE_L6_FORCE __host__ __device__ __forceinline__
#else
#define KPE_L6_FN static inline
#define KPE_L6_FORCE static inline
#endif
// Capability-set violation bits (computed per block into LDS from the capset dictionary)
#define CS_BASE 1u  // add has a capability outside the baseline allow-list
#define CS_DROP 2u  // drop lacks "ALL" (also: no capabilities at all)
#define CS_ADD 4u   // add has anything but NET_BIND_SERVICE

// PSA versioned checks for one pod (PSA v0.29 policy/check_*.go, restated in
// oracle/pss.hpp) from the pod word and the OR of its containers' state bitmaps.
// "Containers" = initContainers + containers + ephemeralContainers.
KPE_L6_FORCE uint32_t cv_fails(uint32_t pw, uint32_t xo, uint32_t co, bool sec_ann_bad,
                                             bool vol_hostpath, bool vol_restricted, uint32_t sys_bad,
                                             bool apparmor_bad, bool sec_pod_ann_bad) {
  // Branch-free: every condition is a 0/1 value combined with & and | (no short circuit), so the
  // whole function is selects and shifts on the lane.
  auto on = [](uint32_t c, uint32_t cv) -> uint32_t { return (c ? 1u : 0u) << cv; };
  const uint32_t nwin = FIELD(pw, P_OS_SH, 2) == OS_WINDOWS ? 0u : ~0u;
  uint32_t f = 0;
  // allowPrivilegeEscalation: some container whose APE is unset (or SC nil) or true
  f |= (xo & (CX_APE_T | CX_APE_U)) ? (1u << CV_APE_1_8) | ((1u << CV_APE_1_25) & nwin) : 0u;
  f |= on(apparmor_bad, CV_APPARMOR_1_0);
  f |= on(co & CS_BASE, CV_CAPS_BASELINE_1_0);
  f |= (co & (CS_DROP | CS_ADD)) ? (1u << CV_CAPS_RESTRICTED_1_22) | ((1u << CV_CAPS_RESTRICTED_1_25) & nwin) : 0u;
  f |= on(pw & (P_HOSTNET | P_HOSTPID | P_HOSTIPC), CV_HOST_NS_1_0);
  f |= on(vol_hostpath, CV_HOST_PATH_1_0);
  f |= on(xo & CX_HOSTPORT, CV_HOST_PORTS_1_0);
  f |= on(xo & CX_PRIV_T, CV_PRIVILEGED_1_0);
  f |= on(xo & CX_PM_OTHER, CV_PROC_MOUNT_1_0);
  f |= on(vol_restricted, CV_RESTRICTED_VOLUMES_1_0);
  const uint32_t prnr = FIELD(pw, P_RNR_SH, 2);
  f |= on((uint32_t)(prnr == TRI_FALSE) | (uint32_t)((xo & CX_RNR_F) != 0u) |
              ((uint32_t)(prnr != TRI_TRUE) & (uint32_t)((xo & CX_RNR_U) != 0u)),
          CV_RUN_AS_NON_ROOT_1_0);
  f |= on((uint32_t)(FIELD(pw, P_RAU_SH, 2) == RAU_ZERO) | (uint32_t)((xo & CX_RAU_Z) != 0u), CV_RUN_AS_USER_1_23);
  const uint32_t psel = FIELD(pw, P_SEL_SH, 3);
  f |= on(((uint32_t)(psel != SEL_NONE) &
           ((uint32_t)(psel == SEL_OTHER) | (uint32_t)((pw & (P_SEL_USER | P_SEL_ROLE)) != 0u))) |
              (uint32_t)((xo & (CX_SEL_OTHER | CX_SEL_USER | CX_SEL_ROLE)) != 0u),
          CV_SELINUX_1_0);
  f |= on((uint32_t)sec_pod_ann_bad | (uint32_t)sec_ann_bad, CV_SECCOMP_BASELINE_1_0);
  // pod seccomp type: valid = RuntimeDefault | Localhost, bad = set and not valid
  const uint32_t psec = FIELD(pw, P_SECCOMP_SH, 3);
  constexpr uint32_t kSecValid = (1u << SECCOMP_RUNTIMEDEFAULT) | (1u << SECCOMP_LOCALHOST);
  constexpr uint32_t kSecBad = 0xFFu & ~kSecValid & ~(1u << SECCOMP_NONE);
  const uint32_t psec_valid = (kSecValid >> psec) & 1u, psec_bad = (kSecBad >> psec) & 1u;
  const uint32_t sec_b = psec_bad | (uint32_t)((xo & (CX_SEC_UNC | CX_SEC_OTHER)) != 0u);
  f |= on(sec_b, CV_SECCOMP_BASELINE_1_19);
  f |= (sec_b | ((psec_valid ^ 1u) & (uint32_t)((xo & CX_SEC_NONE) != 0u)))
           ? (1u << CV_SECCOMP_RESTRICTED_1_19) | ((1u << CV_SECCOMP_RESTRICTED_1_25) & nwin)
           : 0u;
  f |= on(sys_bad & 1u, CV_SYSCTLS_1_0) | on(sys_bad & 2u, CV_SYSCTLS_1_27) | on(sys_bad & 4u, CV_SYSCTLS_1_29);
  f |= on((uint32_t)(FIELD(pw, P_WHP_SH, 2) == TRI_TRUE) | (uint32_t)((xo & CX_WHP_T) != 0u), CV_WIN_HOST_PROCESS_1_0);
  return f;
}
// The pod word's part of the evidence word: bits to set and container bits to clear.
KPE_L6_FN void kpe_l6_pod_evidence(uint32_t pw, uint32_t* set, uint32_t* clr) {
  const uint32_t prnr = FIELD(pw, P_RNR_SH, 2), psel = FIELD(pw, P_SEL_SH, 3), psec = FIELD(pw, P_SECCOMP_SH, 3);
  const uint32_t kSecValid = (1u << SECCOMP_RUNTIMEDEFAULT) | (1u << SECCOMP_LOCALHOST);
  const uint32_t kSecBad = 0xFFu & ~kSecValid & ~(1u << SECCOMP_NONE);
  const bool sel_bad = psel != SEL_NONE && (psel == SEL_OTHER || (pw & (P_SEL_USER | P_SEL_ROLE)));
  *set = ((pw & (P_HOSTNET | P_HOSTPID | P_HOSTIPC)) ? KPE_L6_EV_HOSTNS : 0u) | (prnr == TRI_FALSE ? CX_RNR_F : 0u) |
         (FIELD(pw, P_RAU_SH, 2) == RAU_ZERO ? CX_RAU_Z : 0u) | (sel_bad ? CX_SEL_OTHER : 0u) |
         (((kSecBad >> psec) & 1u) ? CX_SEC_UNC : 0u) | (FIELD(pw, P_WHP_SH, 2) == TRI_TRUE ? CX_WHP_T : 0u);
  *clr = (prnr == TRI_TRUE ? CX_RNR_U : 0u) | (((kSecValid >> psec) & 1u) ? CX_SEC_NONE : 0u);
}
// Checks marked *nw below apply to a pod unless it is a Windows pod.
KPE_L6_FN bool kpe_l6_not_windows(uint32_t pw) { return FIELD(pw, P_OS_SH, 2) != OS_WINDOWS; }
// The same from a constant table (verdict-only evaluations): every field above lies in bits 1-19
// of the pod word and contributes on its own (the SELinux type with its user / role bits), so
// the pod's bits are the OR of one entry per slice of the pod word: bits 1-7, 8-15 and 16-19.
// An entry holds its slice's set bits, its clear bits (KPE_L6_PT_CLR: no field sets those) and,
// in the slice that holds the OS field, KPE_L6_PT_NW for a pod that is not a Windows pod. Built
// once per device (policy- and corpus-independent) and copied to LDS by every block.
#define KPE_L6_PT_B0 128u   // first entry of the second slice
#define KPE_L6_PT_C0 384u   // first entry of the third slice
#define KPE_L6_PT_WORDS 400u
#define KPE_L6_PT_CLR (CX_RNR_U | CX_SEC_NONE)
#define KPE_L6_PT_NW (1u << 31)
KPE_L6_FN uint32_t kpe_l6_pod_table_word(uint32_t i) {
  const uint32_t pw = i < KPE_L6_PT_B0 ? i << 1 : i < KPE_L6_PT_C0 ? (i - KPE_L6_PT_B0) << 8 : (i - KPE_L6_PT_C0) << 16;
  uint32_t set, clr;
  kpe_l6_pod_evidence(pw, &set, &clr);
  return set | clr | (i >= KPE_L6_PT_C0 && kpe_l6_not_windows(pw) ? KPE_L6_PT_NW : 0u);
}
// tab: the table (LDS, or host memory in the checks); the result is split by kpe_l6_pod_split
KPE_L6_FN uint32_t kpe_l6_pod_lookup(const uint32_t* tab, uint32_t pw) {
  return tab[(pw >> 1) & 127u] | tab[KPE_L6_PT_B0 + ((pw >> 8) & 255u)] | tab[KPE_L6_PT_C0 + ((pw >> 16) & 15u)];
}
// The evidence word of a pod from the OR of its containers (cw), the table word and its list bits.
KPE_L6_FN uint32_t kpe_l6_pod_split(uint32_t cw, uint32_t tw, uint32_t lists) {
  return (cw & ~(tw & KPE_L6_PT_CLR)) | (tw & ~(KPE_L6_PT_CLR | KPE_L6_PT_NW)) | lists;
}
// The OR of a pod's first min(nc, 4) staged containers from the four words at its first slot on.
KPE_L6_FN uint32_t kpe_l6_ctr_or(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, uint32_t nc) {
  return (nc > 0u ? x0 : 0u) | (nc > 1u ? x1 : 0u) | (nc > 2u ? x2 : 0u) | (nc > 3u ? x3 : 0u);
}
// Evidence bits of versioned check cv; *nw: the check does not apply to Windows pods.
static inline uint32_t kpe_l6_evidence(uint32_t cv, bool* nw) {
  *nw = cv == CV_APE_1_25 || cv == CV_CAPS_RESTRICTED_1_25 || cv == CV_SECCOMP_RESTRICTED_1_25;
  switch (cv) {
    case CV_APE_1_8:
    case CV_APE_1_25: return CX_APE_T | CX_APE_U;
    case CV_APPARMOR_1_0: return 1u << KPE_L6_ANN_SH;
    case CV_CAPS_BASELINE_1_0: return 1u << KPE_L6_CAP_SH;
    case CV_CAPS_RESTRICTED_1_22:
    case CV_CAPS_RESTRICTED_1_25: return 6u << KPE_L6_CAP_SH;
    case CV_HOST_NS_1_0: return KPE_L6_EV_HOSTNS;
    case CV_HOST_PATH_1_0: return 1u << KPE_L6_VOL_SH;
    case CV_HOST_PORTS_1_0: return CX_HOSTPORT;
    case CV_PRIVILEGED_1_0: return CX_PRIV_T;
    case CV_PROC_MOUNT_1_0: return CX_PM_OTHER;
    case CV_RESTRICTED_VOLUMES_1_0: return 2u << KPE_L6_VOL_SH;
    case CV_RUN_AS_NON_ROOT_1_0: return CX_RNR_F | CX_RNR_U;
    case CV_RUN_AS_USER_1_23: return CX_RAU_Z;
    case CV_SELINUX_1_0: return CX_SEL_OTHER | CX_SEL_USER | CX_SEL_ROLE;
    case CV_SECCOMP_BASELINE_1_0: return (2u << KPE_L6_ANN_SH) | (1u << KPE_L6_SANN_SH);
    case CV_SECCOMP_BASELINE_1_19: return CX_SEC_UNC | CX_SEC_OTHER;
    case CV_SECCOMP_RESTRICTED_1_19:
    case CV_SECCOMP_RESTRICTED_1_25: return CX_SEC_UNC | CX_SEC_OTHER | CX_SEC_NONE;
    case CV_SYSCTLS_1_0: return KPE_L6_EV_SYS0;
    case CV_SYSCTLS_1_27: return KPE_L6_EV_SYS1;
    case CV_SYSCTLS_1_29: return KPE_L6_EV_SYS2;
    case CV_WIN_HOST_PROCESS_1_0: return CX_WHP_T;
    default: return 0u;
  }
}
// The masks of a version class with the versioned checks `checks` (LeanBatchArgs::cls_ev,
// cls_ev_nw): a pod fails the class when its evidence word meets ev, or ev_nw on a pod that is
// not a Windows pod.
struct KpeL6ClassMasks {
  uint32_t ev, ev_nw;
};
static inline KpeL6ClassMasks kpe_l6_class_masks(uint32_t checks) {
  KpeL6ClassMasks m = {0u, 0u};
  for (uint32_t v = 0; v < KPE_NUM_CV; ++v) {
    if (!((checks >> v) & 1u)) continue;
    bool nw;
    const uint32_t ev = kpe_l6_evidence(v, &nw);
    (nw ? m.ev_nw : m.ev) |= ev;
  }
  return m;
}

// ---- the compact columns (DeviceCorpus rec12 / cw4, built once per corpus by
// kpe_lean_pack_kernel) and the packed numbering the verdict-only evaluation decides in ----------
// rec12: words {x, y, z} of a pod record (w, the namespace id, is not read). cw4: one word per
// container, a lossless re-packing of what the LEAN evaluation reads of its record: the
// KPE_L6_CX_USED state bits squeezed together in ascending CX_* order (bits 0-14), the
// capability-set id (bits 15-25) and bit 31, set for every real container: an empty slot is the
// word 0, a container none of whose used states is set is not. No code, no evidence, nothing of
// a policy: the codes are looked up from the id by every evaluation, as from the wide record.
#define KPE_L6C_STATES 15u
#define KPE_L6C_ID_SH 15
#define KPE_L6C_ID_MASK 0x7FFu
#define KPE_L6C_REAL (1u << 31)
static_assert(KPE_MAX_CAPSETS <= KPE_L6C_ID_MASK + 1u, "capability-set ids past the container word's 11 bits");
// The packed evidence word: the in-place word (above) under one fixed permutation of its bits
// (kpe_l6_pack_ev), so every bit keeps its one definition (kpe_l6_evidence, kpe_l6_pod_evidence,
// KPE_L6_PT_CLR) and the packed class masks and pod table are those, permuted. The staged
// container word is (cw4 & states) | capability-set code << CAP_SH | seccomp annotation << SANN_SH.
#define KPE_L6C_CAP_SH 15     // 3 bits, from KPE_L6_CAP_SH
#define KPE_L6C_SANN_SH 18    // 1 bit, from KPE_L6_SANN_SH
#define KPE_L6C_SYS_SH 19     // the sysctl code as it is: bit v from KPE_L6_EV_SYSv
#define KPE_L6C_HOSTNS_SH 22  // from KPE_L6_EV_HOSTNS
#define KPE_L6C_VOL_SH 23     // 2 bits, from KPE_L6_VOL_SH
#define KPE_L6C_ANN_SH 25     // 2 bits, from KPE_L6_ANN_SH; bit 31 (KPE_L6_PT_NW) stays
// the used state bits of cx, squeezed together in ascending order
KPE_L6_FN uint32_t kpe_l6_pack_cx(uint32_t cx) {
  uint32_t p = 0, k = 0;
  for (uint32_t b = 0; b < 32u; ++b)
    if ((KPE_L6_CX_USED >> b) & 1u) p |= ((cx >> b) & 1u) << k++;
  return p;
}
KPE_L6_FN uint32_t kpe_l6_unpack_cx(uint32_t p) {
  uint32_t cx = 0, k = 0;
  for (uint32_t b = 0; b < 32u; ++b)
    if ((KPE_L6_CX_USED >> b) & 1u) cx |= ((p >> k++) & 1u) << b;
  return cx;
}
// the container word of a container record (cx: state bits, cy: CY_* word)
KPE_L6_FN uint32_t kpe_l6_pack_ctr(uint32_t cx, uint32_t cy) {
  return kpe_l6_pack_cx(cx) | ((CY_CAPSET(cy) & KPE_L6C_ID_MASK) << KPE_L6C_ID_SH) | KPE_L6C_REAL;
}
KPE_L6_FN uint32_t kpe_l6_ctr_capset(uint32_t w) { return (w >> KPE_L6C_ID_SH) & KPE_L6C_ID_MASK; }
KPE_L6_FN uint32_t kpe_l6_ctr_states(uint32_t w) { return kpe_l6_unpack_cx(w & ((1u << KPE_L6C_STATES) - 1u)); }
// an in-place evidence word, class mask or pod-table word in the packed numbering
KPE_L6_FN uint32_t kpe_l6_pack_ev(uint32_t ev) {
  const uint32_t sys = ((ev & KPE_L6_EV_SYS0) ? 1u : 0u) | ((ev & KPE_L6_EV_SYS1) ? 2u : 0u) | ((ev & KPE_L6_EV_SYS2) ? 4u : 0u);
  return kpe_l6_pack_cx(ev) | (((ev >> KPE_L6_CAP_SH) & 7u) << KPE_L6C_CAP_SH) |
         (((ev >> KPE_L6_SANN_SH) & 1u) << KPE_L6C_SANN_SH) | (sys << KPE_L6C_SYS_SH) |
         ((ev & KPE_L6_EV_HOSTNS) ? 1u << KPE_L6C_HOSTNS_SH : 0u) | (((ev >> KPE_L6_VOL_SH) & 3u) << KPE_L6C_VOL_SH) |
         (((ev >> KPE_L6_ANN_SH) & 3u) << KPE_L6C_ANN_SH) | (ev & KPE_L6_PT_NW);
}
// KPE_L6_PT_CLR packed (CX_RNR_U, CX_SEC_NONE): bits 4 and 6 of the 15 states
#define KPE_L6C_PT_CLR 0x50u
// kpe_l6_pod_split in the packed numbering (tw: a packed table word)
KPE_L6_FN uint32_t kpe_l6c_pod_split(uint32_t cw, uint32_t tw, uint32_t lists) {
  return (cw & ~(tw & KPE_L6C_PT_CLR)) | (tw & ~(KPE_L6C_PT_CLR | KPE_L6_PT_NW)) | lists;
}
// ---- the pod word column pw4 (DeviceCorpus pw4, written by kpe_lean_pack_kernel beside rec12):
// what the scatter form reads of a pod record, in one word. Of x that is bits 1-22 (the three
// slices kpe_l6_pod_lookup indexes with, the class at PR_CLASS_SH and PR_DECODE_ERR), of y the
// kind id; the packed counts z are not read at all. Layout only, as rec12: no code, no evidence,
// nothing of a policy. Built for a corpus whose kind dictionary has at most KPE_L6P_MAX_KINDS
// entries (the kind id's 10 bits); any other corpus keeps rec12 alone.
//   table slices 0-6, 7-14, 15-18   class 19-20   decode error 21   kind id 22-31
#define KPE_L6P_X_BITS 22u
#define KPE_L6P_B_SH 7
#define KPE_L6P_C_SH 15
#define KPE_L6P_CLASS_SH 19
#define KPE_L6P_DECODE_ERR (1u << 21)
#define KPE_L6P_KIND_SH 22
#define KPE_L6P_MAX_KINDS 1024u
static_assert(P_HOSTNET == (1u << 1) && P_OS_SH + 2 == 20 && P_SECCOMP_SH == KPE_L6P_B_SH + 1 && P_WHP_SH == KPE_L6P_C_SH + 1,
              "pw4's table slices are bits 1-7, 8-15 and 16-19 of the pod word, shifted down by one");
static_assert(PR_CLASS_SH == KPE_L6P_CLASS_SH + 1 && R_CLASS_MASK == 3u && PR_DECODE_ERR == (KPE_L6P_DECODE_ERR << 1) &&
                  KPE_L6P_KIND_SH == KPE_L6P_X_BITS,
              "pw4's class and decode error are bits 20-22 of the pod word, shifted down by one");
KPE_L6_FN uint32_t kpe_l6_pack_pod(uint32_t x, uint32_t y) {
  return ((x >> 1) & ((1u << KPE_L6P_X_BITS) - 1u)) | (GVK_KIND(y) << KPE_L6P_KIND_SH);
}
// kpe_l6_pod_lookup of the pod word a pw4 word was packed from
KPE_L6_FN uint32_t kpe_l6p_pod_lookup(const uint32_t* tab, uint32_t w) {
  return tab[w & 127u] | tab[KPE_L6_PT_B0 + ((w >> KPE_L6P_B_SH) & 255u)] | tab[KPE_L6_PT_C0 + ((w >> KPE_L6P_C_SH) & 15u)];
}
KPE_L6_FN uint32_t kpe_l6p_class(uint32_t w) { return (w >> KPE_L6P_CLASS_SH) & R_CLASS_MASK; }
KPE_L6_FN uint32_t kpe_l6p_kind(uint32_t w) { return w >> KPE_L6P_KIND_SH; }
// kpe_lean_pack_kernel: the compact columns of a corpus, one launch (threads over pods and containers)
struct LeanPackArgs {
  const uint32_t *rec, *crec;  // n x 4 words, nctr x 2 words
  uint32_t *rec12, *cw4;       // out: n x 3 words, nctr words (cw4 null: not built)
  uint32_t* pw4;               // out: n words (null: not built, more than KPE_L6P_MAX_KINDS kinds)
  uint32_t n, nctr;
};

// ---- the owner-tagged columns (DeviceCorpus tag, built once per corpus by kpe_lean_tag_kernel):
// what the scatter form of the compact verdict-only evaluation reads instead of cw4 and the
// volume, sysctl and annotation columns. Every list item carries its owner, the index of its pod
// in the pod's 64-pod tile (row & 63), in bits 26-31 of its first word, so the lane that loaded an
// item can OR the item's evidence into its pod's word without knowing the pod's offsets. Volume,
// sysctl and annotation items also carry their quarter, the pod's tile within its group of four
// consecutive tiles (tile & 3), in bits 24-25: byte 3 of the word is then 4 * owner + quarter,
// the pod's index in the 256 interleaved words of a wave that evaluates the four tiles as one
// group (lean.inl l6_group_tiles). The per-tile forms read the owner alone. Owner and quarter are
// layout (CSR to COO): no code, no evidence, nothing of a policy. A list slot is an item of the
// tile (of the group) when its index is below the tile's (the group's) item count; there is no
// "real" bit.
//   container word   states 0-14 and capability-set id 15-25 as in cw4, owner 26-31 (no quarter:
//                    the word is full)
//   sysctl word      id | quarter << 24 | owner << 26
//   annotation pair  {key id | quarter << 24 | owner << 26, value id}
//   volume word      the source as KPE_L6T_VOL_*, quarter 24-25, owner 26-31
// Ids are masked to 24 bits: KPE_NO_STR stays past every dictionary below 2^24 - 1 entries, and a
// corpus with a larger sysctl or annotation-key dictionary keeps cw4 and the gather form.
#define KPE_L6T_OWNER_SH 26
#define KPE_L6T_QUARTER_SH 24
#define KPE_L6T_ID_MASK ((1u << KPE_L6T_QUARTER_SH) - 1u)
static_assert((KPE_L6C_ID_MASK << KPE_L6C_ID_SH) < (1u << KPE_L6T_OWNER_SH), "the owner overlaps the capability-set id");
KPE_L6_FN uint32_t kpe_l6_tag_owner(uint32_t w) { return w >> KPE_L6T_OWNER_SH; }
KPE_L6_FN uint32_t kpe_l6_tag_quarter(uint32_t w) { return (w >> KPE_L6T_QUARTER_SH) & 3u; }
// 4 * owner + quarter: byte 3 of a volume, sysctl or annotation-key word
KPE_L6_FN uint32_t kpe_l6_tag_slot(uint32_t w) { return w >> KPE_L6T_QUARTER_SH; }
KPE_L6_FN uint32_t kpe_l6_tag_ctr(uint32_t cx, uint32_t cy, uint32_t owner) {
  return kpe_l6_pack_cx(cx) | ((CY_CAPSET(cy) & KPE_L6C_ID_MASK) << KPE_L6C_ID_SH) | (owner << KPE_L6T_OWNER_SH);
}
// (the builders without a quarter give quarter 0)
KPE_L6_FN uint32_t kpe_l6_tag_id(uint32_t id, uint32_t owner) { return (id & KPE_L6T_ID_MASK) | (owner << KPE_L6T_OWNER_SH); }
KPE_L6_FN uint32_t kpe_l6_tagq_id(uint32_t id, uint32_t owner, uint32_t quarter) {
  return kpe_l6_tag_id(id, owner) | (quarter << KPE_L6T_QUARTER_SH);
}
KPE_L6_FN uint32_t kpe_l6_tag_get_id(uint32_t w) { return w & KPE_L6T_ID_MASK; }
// A volume's source mask (VS_* bits, 29 of them) as an index: a volume with exactly one source
// holds the source's VS_* number, one with none the number 31 (no source has it), and the
// evaluation decides hostPath / outside the restricted set by shifting two constant masks by the
// number (kpe_l6_vol_decide: vol_code of the original mask, still taken per step). A volume with
// several sources has KPE_L6T_VOL_ESC: the evaluation reads its original mask.
#define KPE_L6T_VOL_IDX 31u  // the index field, and the index of a volume with no source
#define KPE_L6T_VOL_ESC (1u << 6)
static_assert(VS_EPHEMERAL < 31, "volume source 31 stands for no source");
KPE_L6_FN uint32_t kpe_l6_tag_vol(uint32_t src, uint32_t owner) {
  const uint32_t w = src == 0u ? KPE_L6T_VOL_IDX : (src & (src - 1u)) == 0u ? (uint32_t)__builtin_ctz(src) : KPE_L6T_VOL_ESC;
  return w | (owner << KPE_L6T_OWNER_SH);
}
KPE_L6_FN uint32_t kpe_l6_tagq_vol(uint32_t src, uint32_t owner, uint32_t quarter) {
  return kpe_l6_tag_vol(src, owner) | (quarter << KPE_L6T_QUARTER_SH);
}
// vol_code (bit 0 hostPath, bit 1 outside the restricted set) of a volume word without KPE_L6T_VOL_ESC
KPE_L6_FN uint32_t kpe_l6_vol_decide(uint32_t w) {
  const uint32_t i = w & KPE_L6T_VOL_IDX;
  return (((1u << VS_HOSTPATH) >> i) & 1u) | (((~(uint32_t)PSS_ALLOWED_VOLUMES >> i) & 1u) << 1);
}
// The four tagged columns in one device allocation (LeanShard::cw4 is its base in a scatter
// launch): containers at 0, then volumes, sysctls and annotation pairs at 256-byte boundaries,
// then KPE_L6T_SLACK bytes that the over-reads of the last tile or group end in (the group form
// loads KPE_L6G_VOL_SETS sets of 64 volume words from a group's first volume on: 1,536 bytes).
#define KPE_L6T_SLACK 2048u
// The group form's 64-slot sets loaded up front per 256-pod group (the rest: a wave-uniform loop).
// A group of the C2 corpus (synth.cpp) averages 344 volumes, 12 sysctls and 77 annotations.
#define KPE_L6G_VOL_SETS 6
#define KPE_L6G_SYS_SETS 1
#define KPE_L6G_ANN_SETS 2
static_assert(KPE_L6G_VOL_SETS * 256u <= KPE_L6T_SLACK && KPE_L6G_ANN_SETS * 512u <= KPE_L6T_SLACK, "slack");
// Per-wave LDS of the group form: 256 evidence words (word 4 * pod + quarter), then the rows.
#define KPE_L6G_ACC_BYTES 1024u
struct KpeL6TagLayout {
  uint64_t o_vol, o_sys, o_ann, bytes;  // byte offsets; bytes: the allocation with its slack
};
KPE_L6_FN KpeL6TagLayout kpe_l6_tag_layout(uint32_t nctr, uint32_t nvol, uint32_t nsys, uint32_t npann) {
  KpeL6TagLayout t;
  t.o_vol = ((uint64_t)nctr * 4u + 255u) & ~(uint64_t)255u;
  t.o_sys = (t.o_vol + (uint64_t)nvol * 4u + 255u) & ~(uint64_t)255u;
  t.o_ann = (t.o_sys + (uint64_t)nsys * 4u + 255u) & ~(uint64_t)255u;
  t.bytes = t.o_ann + (uint64_t)npann * 8u + KPE_L6T_SLACK;
  return t;
}
// kpe_lean_tag_kernel: one wave per 64-pod tile; offsets as in kpe_psum_kernel
struct LeanTagArgs {
  const uint32_t *rec, *hdr, *crec, *vol, *sys, *pann;  // the corpus's PSS columns
  uint32_t* tag;                                        // out: the allocation (kpe_l6_tag_layout)
  uint32_t n, ntiles, nctr, nvol, nsys, npann;
};

// kpe_pattern_kernel arguments (device-resident, one copy per binding)
struct PatArgs {
  int64_t n;
  uint32_t R, npr;                 // rules per row, pattern rules
  const uint32_t* doc;             // document tape (2 words per node)
  const uint64_t* doc_off;         // first node of each resource
  const uint32_t* perm;            // lane -> row: rows by descending tape size (wave-uniform walk lengths)
  const KpeScalar* scal;
  const uint8_t* scal_text;
  const KpePNode* nodes;
  const uint4* members;            // resolved per binding (names -> D_KEY ids + 1)
  const uint32_t* lists;
  const KpeLeaf* leaves;
  const KpeCond* conds;
  const KpePat* pats;              // operand records
  const uint8_t* pat_bytes;
  const uint32_t* roots;           // (node, anchor slots) pairs
  const KpePatRule* rules;
  const uint32_t* col2pr;          // verdict column -> C2P_MAKE(pattern rule index + 1, memo slot), or null
  const uint32_t* pbuf;            // glob member-name bitsets (HBM)
  // pattern variables: per-row values written by kpe_cond_kernel (pvals[row * nvars + slot]),
  // template pieces / texts, and the condition-program constants a value may name
  const uint2* pvals;
  uint32_t nvars, pad_;
  const uint2* ptmpl;
  const uint8_t* ttext;
  const KpeScalar* ctab;
  const uint8_t* ctext;
  uint8_t* verdicts;
  // Leaf table (kpe_leaf_table_kernel, once per binding): a leaf whose result depends only on
  // the scalar (no variables) has a slot, lslot[leaf] (KPE_NO_LSLOT: none), and bit sid of
  // ltab[slot * ltab_words ...] is pattern.Validate of scalar sid against it. Null: no table.
  const uint32_t* lslot;
  uint32_t* ltab;
  uint32_t ltab_words, nkeyd;  // nkeyd: strings of the member-name dictionary (D_KEY)
  // the member-name dictionary (D_KEY): keys named by substituted key templates (PMF_VKEY) are
  // looked up by text
  const uint8_t* key_bytes;
  const uint32_t* key_off;
  // table sizes and an error word: read only by KPE_PATVM_CHECK builds (bounds flags)
  uint32_t nnodes, nmembers, nlists, nleaves, nconds, npats, nroots, npbuf;
  uint64_t nscal, ndoc;
  uint32_t* err;
  // memo slot s's representative pattern rule (any rule of the slot: they share the pattern), or
  // ~0u for an unused slot; kpe_pattern_kernel evaluates a row's slots in slot order
  uint32_t slot_rule[KPE_PAT_MEMO];
  // set to 1 by kpe_pattern_kernel when it marks a cell KPE_DEEP_ (cleared before every launch);
  // kpe_pattern_deep_kernel returns at once while it is 0 (no 1-byte-per-cell rescan); null: none
  uint32_t* deep_any;
};

// kpe_cond_kernel arguments (device-resident, one copy per binding)
struct CondArgs {
  int64_t n;
  uint32_t R, ncr;                 // rules per row, condition rules
  const uint32_t* doc;             // document tape (2 words per entry)
  const uint64_t* doc_off;         // root entry of each resource
  const uint64_t* img_off;         // root entry of each resource's images map (KPE_NO_IMAGES: none)
  const uint32_t* perm;            // lane -> row (PatArgs::perm)
  const KpeScalar* scal;
  const uint8_t* scal_text;
  const uint8_t* key_bytes;        // D_KEY dictionary (keys(@) results)
  const uint32_t* key_off;
  const uint2* ops;                // condition program (program.hpp CondProgram)
  const KpeCExpr* exprs;
  const KpeVTmpl* tmpls;
  const KpeCCond* conds;
  const KpeCBlock* blocks;
  const KpeCForeach* fes;
  const KpeCRule* rules;
  const KpeScalar* ctab;           // constants
  const uint8_t* ctext;
  const uint32_t* clist;
  const uint32_t* fkeys;           // field index -> D_KEY id + 1 (0: absent from the corpus)
  const KpeLeaf* leaves;           // InRange values of set operators (KpeCCond::aux): string-pattern
  const KpeCond* pconds;           // leaves of the pattern program's tables
  const KpePat* pats;
  const uint8_t* pat_bytes;
  const PatArgs* pat;              // the pattern program (foreach pattern / anyPattern entries)
  const uint2* tpieces;            // VT_TMPL pieces (CondProgram::tpieces)
  uint32_t txt, pad2_;             // 1: VT_TMPL templates exist (the kernel's LDS text slots)
  const KpePVar* pvars;            // pattern variable slots (query template, use flags)
  uint2* pvals;                    // their per-row values (PatArgs::pvals), or null
  uint32_t nvars, nmsg;             // pattern variable slots; condition trace slots per row
  uint8_t* verdicts;
  uint32_t* mtrace;                // N x nmsg condition traces (schema.h CT_*), or null
};

// kpe_pssx_kernel arguments (device-resident, one copy per binding): podSecurity rules with
// exclusions, after the scan wrote their plain PSS verdicts.
struct PssxArgs {
  int64_t n;
  uint32_t R, nxr;
  const KpeXRule* rules;
  const KpeXExcl* excl;            // predicate fields resolved to pbuf word indices
  const uint32_t* rec;             // pod records (x = pod word)
  const uint32_t *ctr_off, *vol_off, *sys_off, *pann_off;  // per-pod list offsets (n + 1)
  const uint32_t* crec;            // container records (state bitmap, capset | type << 16)
  const uint32_t* capsets;         // 4 words per capability set
  const uint32_t *c_name, *c_image, *c_sann, *c_sann_key;
  const uint32_t *c_sec_str, *c_pm_str, *c_selt_str, *c_selu_str, *c_selr_str;
  const uint32_t *cport_off, *cport_str;
  const uint32_t *vol_src, *sys_id, *pann_k, *pann_v;
  const uint32_t* p_cold;          // 4 words per pod (D_MISC ids)
  const uint32_t *misc_off, *annv_off, *sysd_off;  // dictionary offsets (empty-string tests)
  const uint32_t* ann_norm;        // D_ANNK id -> normalised-key id
  const uint32_t* rf_ann;          // XRF_ANN text index -> normalised-key id (KPE_NO_STR: none)
  uint32_t key_pod_sec, key_fake_sec;  // D_ANNK ids of the pod / "fake" container seccomp keys
  const uint32_t* pbuf;            // predicate bitsets (global locations)
  uint32_t pp_apparmor_key, pp_apparmor_ok, pp_seccomp_ok, pp_caps_ok, pp_nbs, pp_all;
  uint32_t pp_sysctl[3];
  uint8_t* verdicts;
  uint32_t* masks;                 // n x R failing versioned checks, or null
};
