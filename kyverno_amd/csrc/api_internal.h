// What the C-ABI's translation units share (kpe_api.cpp, api_results.cpp, report.cpp), defined once.
// Host part: the program / corpus handles, the namespace groups and the internals called across
// those files. Device part (KPE_API_HIP defined before the include; kpe_api.cpp and api_results.cpp):
// device buffers, the device handle and the per-device copies of a program and a corpus. report.cpp
// takes the host part only: it sees kpe::DeviceCorpus as an incomplete type and no HIP header.
#pragma once

#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/kpe.h"
#include "corpus.hpp"
#include "program.hpp"

struct kpe_program {
  std::unique_ptr<kpe::Program> p;
};
// Namespace groups of a corpus (kpe_corpus_num_namespaces): the ids of the D_NS dictionary, plus
// one for "" when no row interned it
struct NsGroups {
  std::vector<std::string> names;
  uint32_t empty = 0;  // the group of ""
};
struct kpe_corpus {
  std::unique_ptr<kpe::Corpus> c;
  std::unique_ptr<kpe::DeviceCorpus> d;
  mutable std::mutex ns_mu;
  mutable std::unique_ptr<NsGroups> ns;  // built on first use
  // the retired rows (kpe_corpus_retire_rows), ascending and unique; the set only grows and lives
  // with the handle. The device copy is DeviceCorpus::retired (every upload sends it again).
  std::vector<uint32_t> retired;
  ~kpe_corpus();  // kpe_api.cpp, where kpe::DeviceCorpus is complete
};

namespace kpe {
// sets kpe_last_error's text (thread-local, kpe_api.cpp) and returns s
kpe_status fail(kpe_status s, const std::string& m);

// Defined in report.cpp: kCvCheck[v], the PSA check id of versioned check v; the foreach entry that
// decided a cell, from its trace words; the argument checks and the need tables that
// kpe_report_cells_host and kpe_fetch_report_rows share
extern const uint8_t kCvCheck[KPE_NUM_CV];
int64_t fe_decider(const Program& P, const RuleReport& rr, uint32_t b);
kpe_status report_rows_args(uint32_t flags, const kpe_report_rows* io, bool records);
kpe_status report_need_tables(const kpe_program* prog, uint32_t flags, std::vector<uint8_t>& need);

// the namespace groups of c, built on first use
inline const NsGroups& ns_groups(const kpe_corpus* c) {
  std::lock_guard<std::mutex> lk(c->ns_mu);
  if (!c->ns) {
    auto g = std::make_unique<NsGroups>();
    const kpe::Dict& d = c->c->dict[D_NS];
    for (uint32_t i = 0; i < d.size(); ++i) g->names.emplace_back(d.at(i));
    const int64_t e = d.find("");
    if (e < 0) g->names.emplace_back();
    g->empty = e < 0 ? d.size() : (uint32_t)e;
    c->ns = std::move(g);
  }
  return *c->ns;
}
// The argument checks kpe_corpus_gather and kpe_results_gather share: non-null sources, every pair
// inside its source and on a row that is not retired. listed[t] (when not null): a pair names
// source t, or there is no pair at all.
inline kpe_status gather_args(const char* who, const kpe_corpus* const* srcs, int nsrcs, const uint64_t* pairs,
                              uint64_t npairs, std::vector<uint8_t>* listed) {
  const std::string w(who);
  if (!srcs || nsrcs < 1 || (npairs && !pairs)) return fail(KPE_E_INVALID, w + ": null argument");
  for (int t = 0; t < nsrcs; ++t)
    if (!srcs[t]) return fail(KPE_E_INVALID, w + ": null source");
  if (listed) listed->assign((size_t)nsrcs, npairs ? 0 : 1);
  for (uint64_t k = 0; k < npairs; ++k) {
    const uint64_t t = pairs[2 * k], r = pairs[2 * k + 1];
    if (t >= (uint64_t)nsrcs || r >= (uint64_t)srcs[t]->c->n) return fail(KPE_E_INVALID, w + ": a pair outside its source");
    const auto& ret = srcs[t]->retired;
    if (!ret.empty() && std::binary_search(ret.begin(), ret.end(), (uint32_t)r))
      return fail(KPE_E_INVALID, w + ": a pair names a retired row");
    if (listed) (*listed)[t] = 1;
  }
  return KPE_OK;
}
}  // namespace kpe

#ifdef KPE_API_HIP
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels_abi.h"

#define HIPCHK(x)                                                                                  \
  do {                                                                                             \
    hipError_t e_ = (x);                                                                           \
    if (e_ != hipSuccess) return kpe::fail(KPE_E_DEVICE, std::string(#x ": ") + hipGetErrorString(e_)); \
  } while (0)

#define PCHK(x)                     \
  do {                              \
    hipError_t e_ = (x);            \
    if (e_ != hipSuccess) return e_; \
  } while (0)

namespace kpe {
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t ensure(size_t n) {
    if (n <= bytes && p) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    hipError_t e = hipMalloc(&p, std::max<size_t>(n, 16));
    if (e == hipSuccess) bytes = n;
    return e;
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

template <class T>
hipError_t upload(DevBuf& b, const std::vector<T>& v, hipStream_t s) {
  hipError_t e = b.ensure(v.size() * sizeof(T) + 128);  // + slack: word-wide text compares and the pattern
                                                        // VM's 8-slot body loads read past the end
  if (e != hipSuccess) return e;
  if (!v.empty()) return hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s);
  return hipSuccess;
}

}  // namespace kpe

// Evaluation streams per device: a corpus binding is pinned to one of them, so the
// evaluations of independent corpora (shards, rotated batches) run concurrently and one
// launch's prologue overlaps another's tail. Setup (uploads, binds) and timed launches
// use stream 0.
constexpr int kMaxLanes = 4;
struct kpe_device {
  int ordinal = 0;
  hipStream_t stream = nullptr;  // == lanes[0]
  hipStream_t lanes[kMaxLanes] = {};
  int nlanes = 2;  // KPE_LANES (1..4) overrides
  uint32_t next_lane = 0;
  std::mutex mu;
  bool timing = false;
  struct EvPair {
    hipEvent_t a, b, c, d;
    double bytes, pbytes;
    int kind;        // scan instantiation (kpe_kernel_stats::scan_kernel)
    bool pre, post;  // a kernel ran between a and b (dictionary pass / prologue), c and d (later passes)
  };
  std::vector<EvPair> pending;
  std::vector<hipEvent_t> pool;
  uint64_t launches = 0;
  double pss_ms = 0, dict_ms = 0, pat_ms = 0, last_bytes = 0, last_pbytes = 0, sum_bytes = 0, sum_pbytes = 0;
  double pss_min = 0, pss_max = 0, pss_sq = 0;  // spread of the scan launches' durations
  int last_kind = 0;
  // knobs, read once at kpe_device_open: KPE_NO_BIND_CACHE (recompute per-binding products every
  // evaluation), KPE_PATVM_ERR (report a KPE_PATVM_CHECK build's bounds flags), KPE_LEAN6_MINW /
  // KPE_LEAN6_TPW (waves a LEAN6 launch keeps / tiles per wave, for A/B runs), KPE_LEAN6_SHAPE
  // (A/B runs: bit 0 the instantiation that reads the seccomp annotations, bit 1 the one that
  // decides every versioned check, for programs that need neither; bit 4, i.e. 16: the
  // verdict-only form reads the wide records, not the corpus's compact columns; bit 5, i.e. 32:
  // the compact form gathers each pod's items from rec12 / cw4, not the scatter form over the
  // owner-tagged columns; bit 6, i.e. 64: scatter launches of two or four tiles per wave read
  // rec12 as those of one tile do, not the pod word column pw4; bit 7, i.e. 128: narrow launches
  // of four tiles per wave keep the per-tile form, not the group form)
  bool no_cache = false, patvm_err = false;
  // the general scan of a podSecurity program walks each pod's lists itself; KPE_PSUM=1: it reads
  // per-pod records kpe_psum_kernel builds right before it on the second stream (round 6: C4 step
  // 0.393 ms without them against 0.416 ms with them, C3 unchanged, profiles/r06_n; round 5 kept the
  // records for their 0.92x traffic against 1.98x: profiles/r05_psA, r05_psB, r05_final5)
  bool no_psum = true;
  uint64_t lean_min_waves = 16384;  // 256 CUs x 4 SIMDs x 16 waves
  uint32_t lean_tpw = 0, lean_shape = 0;
  int lean_form = -1;  // what the last kpe_lean6_kernel launch read (kpe_debug_lean_form)
  int lean_narrow = 0;  // and whether it was the narrow scatter form (kpe_debug_lean_narrow)
  int lean_group = 0;   // and whether that was its group form (kpe_debug_lean_group)
  // kpe_lean6_kernel's pod-evidence table (kernels_abi.h kpe_l6_pod_table_word), built at
  // kpe_device_open: it depends on neither the policies nor a corpus
  kpe::DevBuf lean_pod_tab;
  kpe::DevBuf lean_pod_tab_c;  // the same in the packed numbering (kpe_l6_pack_ev): launches over the compact columns
  // pinned staging for corpus uploads (two halves, double-buffered; allocated on first use): a
  // pageable hipMemcpyAsync is staged by the runtime chunk by chunk, a pinned one is one DMA
  static constexpr size_t kStageHalf = 16u << 20;
  char* stage = nullptr;
  hipEvent_t stage_ev[2] = {};
  bool stage_busy[2] = {};
  int stage_cur = 0;
  double up_alloc_s = 0, up_copy_s = 0;  // KPE_DEBUG upload breakdown (under mu)
  // kpe_changed_rows_fp's scratch (the new fingerprints, the row flags, the selection's tiles): 9
  // bytes per row of the largest corpus compared so far, kept between calls (an allocation of
  // that size costs more than the kernels). Used under mu by calls that wait before they return.
  kpe::DevBuf fp_scratch;
  // kpe_fetch_report_rows' scratch, kept between calls for the same reason: the uploaded row list,
  // the compact matrix, the tiles and the tables (rr_scratch), and the gathered lists with their
  // payloads (rr_out), each as large as the largest call so far needed
  kpe::DevBuf rr_scratch, rr_out;
  // kpe_fetch_namespace_counts with timing on: the last call's kernel time (HIP events) and the
  // last rows-by-namespace index build + upload (host clock)
  double ns_kernel_ms = 0, ns_index_ms = 0;
  hipEvent_t get_ev() {
    if (!pool.empty()) {
      hipEvent_t e = pool.back();
      pool.pop_back();
      return e;
    }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
  }
};

namespace kpe {
struct DeviceProgram {
  int ordinal = -1;
  DevBuf rule_exc;  // KpeRule::exc per rule (PolicyExceptions)
  DevBuf rules, rule_lanes, narrow_rules, fmask, narrow_cls, filters, fterms, terms, kindsels, annpairs, selectors, selreqs,
      pat_bytes, pats;
  bool narrow = false;  // per-lane rule loop (kernels_abi.h NR_*)
  bool tt = false;      // + truth-table fast path
  uint32_t ncls = 0, pss_rules = 0, err_rules = 0, pat_rules = 0;
  std::vector<uint32_t> cls_h;  // host copy of narrow_cls: (cv_mask, rule mask) per version class
  // pattern rules: compiled trees + operand records (program.hpp PatProgram)
  DevBuf pnodes, plists, pleaves, pconds, ppats, pbytes, proots, prules;
  DevBuf plslot, pslot_leaf;  // leaf-table slot per leaf, leaf per slot (PatArgs::lslot)
  std::vector<uint32_t> lslot_h;  // host copy of plslot (bound into the scalar-leaf members' w)
  uint32_t nlslots = 0;
  bool ltab_all = false;  // every leaf has a slot or is PL_NEVER: the pattern kernel's LT instance
  DevBuf pvars, ptmpl, ttext;  // pattern variables: slots, template pieces, template texts
  DevBuf pcol2pr;  // verdict column -> pattern rule index + 1 (0: not a pattern rule)
  // condition rules: compiled programs (program.hpp CondProgram)
  DevBuf cops, cexprs, ctmpls, cconds, cblocks, cfes, crules, cconsts, ctext, cclist, ctpieces;
  DevBuf xrules;  // podSecurity rules with exclusions (program.hpp PssxProgram)
  std::vector<uint8_t> pat_bytes_h;
  std::vector<KpePat> pats_h;  // pattern k of predicate p: pats_h[pat0[p] + k]
  std::vector<uint32_t> pat0;
};

struct Binding {  // program x corpus (dictionary sizes decide predicate placement)
  const Program* prog = nullptr;
  DevBuf jobs, pbuf, verdicts, masks, counts_out;
  DevBuf apply_segs;  // ApplyOne policies' rule ranges (uint2 r0, r1)
  uint32_t napply_segs = 0;
  DevBuf dargs;        // device copy of the scan arguments (kernel reads them with scalar loads)
  DevBuf zero_page;    // 256 zero bytes (loads of columns a program does not read)
  DevBuf fuse;         // fused dictionary pass image (pairs, patterns, small dictionaries)
  uint32_t fuse_lds = 0, fuse_words = 0, npairs = 0, fuse_pats = 0, fuse_patb = 0;
  DevBuf pmembers, pargs, perr, pdeep;  // pattern rules: resolved members, PatArgs copy, check flags,
                                        // PatArgs::deep_any
  bool pargs_valid = false;
  DevBuf pvals;  // pattern variables: per-row values (kpe_cond_kernel -> kpe_pattern_kernel)
  DevBuf cfkeys, cargs;  // condition rules: resolved field names, CondArgs copy
  DevBuf mtrace;         // condition traces: N x CondProgram::nmsg words (schema.h CT_*)
  bool cargs_valid = false;
  DevBuf pimg;  // prologue image (kpe_launch_prep)
  // The large-domain predicate bitsets (pbuf) and the prologue image depend only on the
  // program and the corpus dictionaries: computed by the first evaluation of a binding and
  // kept until the binding is rebuilt (KPE_NO_BIND_CACHE=1: recomputed every evaluation).
  bool inv_ready = false;
  uint32_t pimg_words = 0, capb_lds = 0;
  size_t prep_dyn_bytes = 0;  // the prep kernel's LDS: the scan layout + the fuse area
  bool lean = false;  // LEAN scan instantiation (kind table; no check masks)
  int lean_kind = 0;  // KpeScanKind of the LEAN scan: KPE_SCAN_LEAN6 (kpe_lean6_kernel) or KPE_SCAN_LEAN
  int gen_code = 0;   // KpeScanKind of the general scan: WIDE / NARROW, | KPE_SCAN_PSUM with scan records
  uint32_t kt_lds = PRED_NONE, nkinds = 0;
  DevBuf xexcl, ann_norm, rf_ann, xargs;  // podSecurity exclusions: resolved excludes, key tables, PssxArgs
  bool xargs_valid = false;
  void* xmasks = nullptr;  // the masks buffer xargs points at (null: no masks)
  uint32_t xpp[9] = {}, key_pod_sec = KPE_NO_STR, key_fake_sec = KPE_NO_STR;
  ScanArgs hargs{};    // what dargs holds
  bool args_valid = false;
  DevBuf terms_r, kindsels_r, annpairs_r, selectors_r, selreqs_r, cv_classes;  // resolved tables
  // selector requirement masks (ScanArgs::selm): requirement lists per space, the tables
  DevBuf sel_rq, sel_nq, sel_km, sel_vm, sel_nsq;
  DevBuf ltab;  // leaf table (PatArgs::ltab)
  uint32_t ltab_words = 0;
  uint32_t selm = 0, sel_nrq = 0, sel_nnq = 0;
  uint64_t sm[5] = {};  // pos (EQ / In), wild, NotIn, Exists, DoesNotExist
  uint32_t pp[10] = {};  // fixed PSS predicate locations
  uint32_t wave_lds = 0, wave_words = 0, filt_lds = PRED_NONE, fterm_lds = 0, tt_lds = PRED_NONE;
  uint32_t selt_lds = PRED_NONE;  // ScanArgs::selt_lds
  uint32_t kslot_lds = PRED_NONE, nkslot_g = 0;  // ScanArgs::kslot_lds / nkslot_g
  DevBuf kslot_tab;
  size_t dyn_bytes = 0;
  uint32_t nblocks = 0, njobs = 0, blob_words = 0, scan_blocks = 0;
  uint32_t need = 0;
  double scan_bytes = 0;
  size_t cells = 0;
  int lane = -1;                  // evaluation stream (kpe_device::lanes) of this corpus
  hipStream_t last = nullptr;     // stream of the last launch (fetch orders after it)
};

struct DeviceCorpus {
  int ordinal = -1;
  DevBuf dict_bytes[KPE_NUM_DOMAINS], dict_off[KPE_NUM_DOMAINS];
  DevBuf r_gvk, r_name, r_mns, r_nsa, ann_off, ann_k, ann_v;
  DevBuf lab_off, lab_k, lab_v, r_nsl, nsl_off, nsl_k, nsl_v;
  DevBuf rec, hdr, crec, vol_src, sys_id, pann_kv, c_sann, capsets;
  DevBuf doc, doc_off, img_off, scal, scal_text;  // document tape + scalar table (pattern rules)
  DevBuf doc_perm;  // rows by descending tape size: the pattern / condition kernels' lane -> row map
  DevBuf limit_rows;                     // rows past a per-resource limit
  DevBuf retired;                        // kpe_corpus::retired (kpe_retire_rows_kernel reads it last)
  DevBuf nsl_map;  // kpe_corpus_set_namespace_labels: namespace id -> table row (kpe_nsl_remap_kernel's input)
  // cold pod columns, uploaded on the first binding of a program with podSecurity exclusions
  DevBuf ctr_off, vol_off, sys_off, pann_off, c_name, c_image, c_sann_key, c_sec_str, c_pm_str, c_selt_str, c_selu_str,
      c_selr_str, cport_off, cport_str, pann_k, pann_v, p_cold;
  bool cold = false;
  // PSA dictionary codes (kpe_psa_codes_kernel; policy-independent, per distinct string), built at
  // the first binding of a podSecurity program; psum: the general scan's per-pod records, scratch
  // rebuilt by every evaluation that reads them (kpe_psum_kernel)
  DevBuf psum, psa_codes, psa_fixed;
  PsaCodes psa_L{};
  bool codes_ready = false;
  // the LEAN evaluation's compact columns (kpe_lean_pack_kernel: 12-byte pod records, one word
  // per container; kernels_abi.h), built with the codes for a corpus whose binding is LEAN6
  DevBuf rec12, cw4;
  bool pack_ready = false;
  // the pod word column (kernels_abi.h kpe_l6_pack_pod), written beside rec12 for a corpus of at
  // most KPE_L6P_MAX_KINDS kinds: what scatter launches of two or four tiles per wave read of a pod
  DevBuf pw4;
  bool pw4_ready = false;
  // its owner-tagged columns (kpe_lean_tag_kernel: one allocation, kernels_abi.h kpe_l6_tag_layout),
  // read by the scatter form of the compact evaluation. A device builds these or cw4, whichever
  // its selected shape reads (KPE_LEAN6_SHAPE bit 5); a corpus they cannot hold keeps cw4.
  DevBuf tag;
  bool tag_ready = false, cw4_ready = false;
  Binding bind;
  bool has_masks = false;
  // rows by namespace group (kpe_fetch_namespace_counts): row ids sorted by group, the groups'
  // work items (kernels_abi.h KpeNsItem), and on the host the first item of each group (G + 1)
  DevBuf ns_rows, ns_items;
  DevBuf ns_out;  // the counters of a small window (kpe_fetch_namespace_counts keeps up to 4 MiB)
  std::vector<uint64_t> ns_item_off;
  bool ns_ready = false;
  // the kept result (kpe_results_keep): a copy of one evaluation's N x kept_rules verdict matrix and
  // its rules' names. It belongs to the corpus, not to the binding: the next program's bind leaves it.
  DevBuf kept;
  int64_t kept_rules = -1;  // -1: nothing kept
  std::vector<std::string> kept_names;
  // kpe_results_splice: the second matrix buffer (K' is written there and the two swap, the old one
  // stays as the spare of the next splice) and the row flags of the last splice (N bytes, valid
  // until the next splice, keep, drop or upload; kpe_spliced_rows reads them)
  DevBuf kept_spare, splice_flags;
  bool splice_valid = false;
  // the kept fingerprints (kpe_fingerprints_keep / _load): 8 bytes per row, independent of `kept`
  DevBuf fps;
  std::vector<uint64_t> fps_tbl;  // host bytes of the last keep's salt table (its copy is enqueued)
  bool fps_kept = false;
};
}  // namespace kpe
#endif  // KPE_API_HIP
