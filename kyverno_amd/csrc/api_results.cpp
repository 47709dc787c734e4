// C-ABI implementation (include/kpe.h): the fetches from a finished evaluation. Cell selection and
// row summaries, result deltas, row fingerprints, namespace groups and counts, pattern and condition
// traces, the report detail of a row list. Each family is a few device launches with its host
// mirror (`_host`) beside it.
#define KPE_API_HIP
#include <algorithm>
#include <chrono>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "api_internal.h"
#include "kernels_launch.h"

using kpe::DevBuf;
using kpe::fail;
using kpe::fe_decider;
using kpe::ns_groups;
using kpe::report_need_tables;
using kpe::report_rows_args;

static_assert(KPE_CTRACE_WORDS == 4u && KPE_FE_TRACE_WORDS == KPE_CTRACE_WORDS, "four condition words per cell");
static_assert(sizeof(uint4) == KPE_FE_TRACE_WORDS * 4u, "a foreach cell's words are one uint4");

extern "C" {

// ---- sparse result fetch: cell selection and row summaries ------------------------------------
static kpe_status select_impl(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, const uint8_t* sel,
                              uint64_t* cells_out, uint8_t* verdicts_out, uint64_t cap, uint64_t* total_out) {
  *total_out = 0;
  if (!dev || !prog || !c || !sel) return fail(KPE_E_INVALID, "null argument");
  if (cap && !cells_out) return fail(KPE_E_INVALID, "cap > 0 without a cells buffer");
  const size_t R = prog->p->rules.size();
  const uint64_t cells = (uint64_t)c->c->n * R;
  if (!cells) return KPE_OK;
  if (!c->d) return fail(KPE_E_STATE, "corpus not uploaded");
  std::lock_guard<std::mutex> lk(dev->mu);
  HIPCHK(hipSetDevice(dev->ordinal));
  auto& B = c->d->bind;
  if (B.prog != prog->p.get()) return fail(KPE_E_STATE, "no evaluation of this program on this corpus");
  if (c->d->ordinal != dev->ordinal) return fail(KPE_E_STATE, "corpus not uploaded to this device");
  hipStream_t s = B.last ? B.last : dev->stream;
  // scratch of this call (freed on every return path): tile offsets, tile counts, the masks
  const uint64_t ntiles = (cells + 4095u) / 4096u;
  const size_t off_bytes = (size_t)((ntiles + 2) & ~(uint64_t)1) * 8;  // + the total, kept 16-byte aligned
  const size_t cnt_bytes = (size_t)((ntiles + 3) & ~(uint64_t)3) * 4;  // read four at a time
  DevBuf scratch, dcells, dverd;
  HIPCHK(scratch.ensure(off_bytes + cnt_bytes + R));
  uint64_t* d_off = scratch.as<uint64_t>();
  uint32_t* d_cnt = reinterpret_cast<uint32_t*>(scratch.as<uint8_t>() + off_bytes);
  uint8_t* d_sel = scratch.as<uint8_t>() + off_bytes + cnt_bytes;
  HIPCHK(hipMemcpyAsync(d_sel, sel, R, hipMemcpyHostToDevice, s));
  int na_sel = 0;  // most cells of a wide matrix are KPE_NA: the kernels pass over them unless a mask selects them
  for (size_t r = 0; r < R; ++r) na_sel |= sel[r] & 1;
  HIPCHK(kpe_launch_select_count(B.verdicts.as<uint8_t>(), cells, (uint32_t)R, d_sel, na_sel, d_cnt, d_off, s));
  uint64_t total = 0;
  HIPCHK(hipMemcpyAsync(&total, d_off + ntiles, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *total_out = total;
  const uint64_t m = std::min(total, cap);
  if (!m) return KPE_OK;
  // staging sized by what is written, not by cap
  HIPCHK(dcells.ensure((size_t)m * 8));
  if (verdicts_out) HIPCHK(dverd.ensure((size_t)m));
  HIPCHK(kpe_launch_select_scatter(B.verdicts.as<uint8_t>(), cells, (uint32_t)R, d_sel, na_sel, d_off, m,
                                   dcells.as<uint64_t>(), verdicts_out ? dverd.as<uint8_t>() : nullptr, s));
  HIPCHK(hipMemcpyAsync(cells_out, dcells.p, (size_t)m * 8, hipMemcpyDeviceToHost, s));
  if (verdicts_out) HIPCHK(hipMemcpyAsync(verdicts_out, dverd.p, (size_t)m, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return KPE_OK;
}

int64_t kpe_select_cells(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, const uint8_t* sel,
                         uint64_t* cells, uint8_t* verdicts_out, uint64_t cap) {
  uint64_t total = 0;
  const kpe_status st = select_impl(dev, prog, c, sel, cells, verdicts_out, cap, &total);
  return st ? -(int64_t)st : (int64_t)total;
}

// the counter of a verdict cell (results.go:39-55; an unscored fail is a warn, :131-133)
static inline void summary_add(kpe_row_summary& o, uint8_t v, bool scored) {
  switch (v) {
    case KPE_PASS: ++o.pass; break;
    case KPE_FAIL: ++(scored ? o.fail : o.warn); break;
    case KPE_WARN: ++o.warn; break;
    case KPE_ERROR: ++o.error; break;
    case KPE_SKIP: ++o.skip; break;
    case KPE_UNDECIDED: ++o.undecided; break;
    default: break;  // KPE_NA: no RuleResponse
  }
}

kpe_status kpe_row_summaries_host(const kpe_program* prog, const uint8_t* verdicts, uint64_t nrows,
                                  kpe_row_summary* out) {
  if (!prog || (nrows && (!verdicts || !out))) return fail(KPE_E_INVALID, "null argument");
  const kpe::Program& P = *prog->p;
  const size_t R = P.rules.size();
  if (R > 65535) return fail(KPE_E_LIMIT, "row summaries count at most 65535 rules");
  for (uint64_t i = 0; i < nrows; ++i) {
    kpe_row_summary o{};
    for (size_t r = 0; r < R; ++r) summary_add(o, verdicts[i * R + r], P.reports[r].scored);
    out[i] = o;
  }
  return KPE_OK;
}

kpe_status kpe_fetch_row_summaries(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, uint64_t row0,
                                   uint64_t nrows, kpe_row_summary* out) {
  if (!dev || !prog || !c || (nrows && !out)) return fail(KPE_E_INVALID, "null argument");
  const kpe::Program& P = *prog->p;
  const size_t R = P.rules.size();
  if (R > 65535) return fail(KPE_E_LIMIT, "row summaries count at most 65535 rules");
  if (row0 > (uint64_t)c->c->n || nrows > (uint64_t)c->c->n - row0) return fail(KPE_E_INVALID, "rows past the corpus");
  if (!nrows) return KPE_OK;
  if (!R) {
    memset(out, 0, nrows * sizeof(kpe_row_summary));
    return KPE_OK;
  }
  if (!c->d) return fail(KPE_E_STATE, "corpus not uploaded");
  std::lock_guard<std::mutex> lk(dev->mu);
  HIPCHK(hipSetDevice(dev->ordinal));
  auto& B = c->d->bind;
  if (B.prog != prog->p.get()) return fail(KPE_E_STATE, "no evaluation of this program on this corpus");
  if (c->d->ordinal != dev->ordinal) return fail(KPE_E_STATE, "corpus not uploaded to this device");
  hipStream_t s = B.last ? B.last : dev->stream;
  std::vector<uint8_t> unscored(R);
  for (size_t r = 0; r < R; ++r) unscored[r] = P.reports[r].scored ? 0 : 1;
  static_assert(sizeof(kpe_row_summary) == 12, "3 words per row");
  const size_t out_bytes = (size_t)nrows * sizeof(kpe_row_summary);
  DevBuf scratch;  // this call's: the rows' summaries, then the unscored flags
  HIPCHK(scratch.ensure(out_bytes + R));
  uint8_t* d_uns = scratch.as<uint8_t>() + out_bytes;
  HIPCHK(hipMemcpyAsync(d_uns, unscored.data(), R, hipMemcpyHostToDevice, s));
  HIPCHK(kpe_launch_row_summary(B.verdicts.as<uint8_t>(), (uint32_t)R, row0, nrows, d_uns, scratch.as<uint32_t>(), s));
  HIPCHK(hipMemcpyAsync(out, scratch.p, out_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return KPE_OK;
}

// ---- result deltas: a kept matrix per corpus, changed rows, transition tables ------------------
kpe_status kpe_results_keep(kpe_device* dev, const kpe_program* prog, kpe_corpus* c) {
  if (!dev || !prog || !c) return fail(KPE_E_INVALID, "null argument");
  if (!c->d) return fail(KPE_E_STATE, "corpus not uploaded");
  std::lock_guard<std::mutex> lk(dev->mu);
  HIPCHK(hipSetDevice(dev->ordinal));
  kpe::DeviceCorpus& D = *c->d;
  auto& B = D.bind;
  if (B.prog != prog->p.get()) return fail(KPE_E_STATE, "no evaluation of this program on this corpus");
  if (D.ordinal != dev->ordinal) return fail(KPE_E_STATE, "corpus not uploaded to this device");
  const kpe::Program& P = *prog->p;
  const size_t R = P.rules.size();
  const size_t cells = (size_t)c->c->n * R;
  D.kept_rules = -1;
  D.splice_valid = false;
  HIPCHK(D.kept.ensure(cells));
  // on the stream of the evaluation: after it, and before the corpus's next one (launch() keeps a
  // corpus's launches ordered and a rebind waits for B.last)
  hipStream_t s = B.last ? B.last : dev->stream;
  if (cells) HIPCHK(hipMemcpyAsync(D.kept.p, B.verdicts.p, cells, hipMemcpyDeviceToDevice, s));
  D.kept_names.assign(P.rule_names.begin(), P.rule_names.end());
  D.kept_names.resize(R);
  D.kept_rules = (int64_t)R;
  return KPE_OK;
}

kpe_status kpe_results_drop(kpe_device* dev, kpe_corpus* c) {
  if (!dev || !c) return fail(KPE_E_INVALID, "null argument");
  if (!c->d) return KPE_OK;
  std::lock_guard<std::mutex> lk(dev->mu);
  HIPCHK(hipSetDevice(dev->ordinal));
  kpe::DeviceCorpus& D = *c->d;
  D.kept_rules = -1;
  D.kept_names.clear();
  if (D.kept.p) HIPCHK(hipFree(D.kept.p));  // waits for the copy
  D.kept.p = nullptr, D.kept.bytes = 0;
  D.splice_valid = false;
  if (D.kept_spare.p) HIPCHK(hipFree(D.kept_spare.p));
  D.kept_spare.p = nullptr, D.kept_spare.bytes = 0;
  if (D.splice_flags.p) HIPCHK(hipFree(D.splice_flags.p));
  D.splice_flags.p = nullptr, D.splice_flags.bytes = 0;
  return KPE_OK;
}

int kpe_results_kept_rules(const kpe_corpus* c) { return c && c->d ? (int)c->d->kept_rules : -1; }
const char* kpe_results_kept_rule_name(const kpe_corpus* c, int r) {
  if (!c || !c->d || r < 0 || r >= c->d->kept_rules) return nullptr;
  return c->d->kept_names[(size_t)r].c_str();
}

kpe_status kpe_delta_column_map(const kpe_corpus* c, const kpe_program* prog, int32_t* old_of) {
  if (!c || !prog) return fail(KPE_E_INVALID, "null argument");
  if (!c->d || c->d->kept_rules < 0) return fail(KPE_E_STATE, "no kept result on this corpus");
  const kpe::Program& P = *prog->p;
  const size_t Rn = P.rules.size();
  if (Rn && !old_of) return fail(KPE_E_INVALID, "null argument");
  std::map<std::string, int32_t> kept;
  for (size_t r = 0; r < c->d->kept_names.size(); ++r)
    if (!kept.emplace(c->d->kept_names[r], (int32_t)r).second)
      return fail(KPE_E_INVALID, "kept rule name occurs twice: " + c->d->kept_names[r]);
  std::map<std::string, int32_t> seen;
  for (size_t r = 0; r < Rn; ++r) {
    const std::string name = r < P.rule_names.size() ? P.rule_names[r] : std::string();
    if (!seen.emplace(name, (int32_t)r).second) return fail(KPE_E_INVALID, "rule name occurs twice: " + name);
    const auto it = kept.find(name);
    old_of[r] = it == kept.end() ? -1 : it->second;
  }
  return KPE_OK;
}

// The map's checks, shared by the device calls and the host twins: every entry is -1 or a kept
// column, and no kept column is named twice. named[o] = 1 for the kept columns the map names.
static kpe_status delta_map_check(const int32_t* old_of, size_t Rn, size_t Ro, std::vector<uint8_t>& named) {
  named.assign(Ro, 0);
  for (size_t r = 0; r < Rn; ++r) {
    const int32_t o = old_of[r];
    if (o == -1) continue;
    if (o < -1 || (size_t)o >= Ro) return fail(KPE_E_INVALID, "column map entry outside the kept rules");
    if (named[(size_t)o]) return fail(KPE_E_INVALID, "column map names a kept column twice");
    named[(size_t)o] = 1;
  }
  return KPE_OK;
}
static inline bool delta_always(const uint8_t* always, size_t r, uint8_t x) {
  return always && x < 8 && ((always[r] >> x) & 1);
}

int64_t kpe_changed_rows_host(const uint8_t* old_v, const uint8_t* new_v, uint64_t n, uint32_t Ro, uint32_t Rn,
                              const int32_t* old_of, const uint8_t* always, uint64_t* rows, uint8_t* verdict_rows,
                              uint64_t cap) {
  if ((Rn && !old_of) || (cap && !rows)) return -(int64_t)fail(KPE_E_INVALID, "null argument");
  if (n && ((Ro && !old_v) || (Rn && !new_v))) return -(int64_t)fail(KPE_E_INVALID, "null argument");
  std::vector<uint8_t> named;
  if (kpe_status st = delta_map_check(old_of, Rn, Ro, named)) return -(int64_t)st;
  std::vector<uint32_t> gone;  // kept columns no entry names
  for (uint32_t o = 0; o < Ro; ++o)
    if (!named[o]) gone.push_back(o);
  uint64_t total = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t* nw = new_v + (size_t)i * Rn;
    const uint8_t* od = old_v + (size_t)i * Ro;
    bool ch = false;
    for (uint32_t r = 0; r < Rn && !ch; ++r) {
      const uint8_t x = nw[r], o = old_of[r] >= 0 ? od[old_of[r]] : (uint8_t)KPE_NA;
      ch = x != o || delta_always(always, r, x);
    }
    for (size_t k = 0; k < gone.size() && !ch; ++k) ch = od[gone[k]] != KPE_NA;
    if (!ch) continue;
    if (total < cap) {
      rows[total] = i;
      if (verdict_rows && Rn) memcpy(verdict_rows + (size_t)total * Rn, nw, Rn);
    }
    ++total;
  }
  return (int64_t)total;
}

kpe_status kpe_delta_transitions_host(const uint8_t* old_v, const uint8_t* new_v, uint64_t n, uint32_t Ro, uint32_t Rn,
                                      const int32_t* old_of, uint64_t* out) {
  if (Rn && (!old_of || !out)) return fail(KPE_E_INVALID, "null argument");
  if (n && ((Ro && !old_v) || (Rn && !new_v))) return fail(KPE_E_INVALID, "null argument");
  std::vector<uint8_t> named;
  if (kpe_status st = delta_map_check(old_of, Rn, Ro, named)) return st;
  if (Rn) memset(out, 0, (size_t)Rn * 64 * sizeof(uint64_t));
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t* nw = new_v + (size_t)i * Rn;
    const uint8_t* od = old_v + (size_t)i * Ro;
    for (uint32_t r = 0; r < Rn; ++r) {  // codes & 7: the alphabet
      const uint32_t o = old_of[r] >= 0 ? od[old_of[r]] & 7u : (uint32_t)KPE_NA;
      ++out[(size_t)r * 64 + o * 8 + (nw[r] & 7u)];
    }
  }
  return KPE_OK;
}

// What kpe_changed_rows and kpe_delta_transitions check before any device call, and the tables
// the kernels read: tab[r] = the kept column of new column r (bits 0-15, 0xFFFF: none) | always[r]
// << 16; unm[o] = 1 for a kept column the map does not name.
static kpe_status delta_tables(const kpe_program* prog, const kpe_corpus* c, const int32_t* old_of, const uint8_t* always,
                               std::vector<uint32_t>& tab, std::vector<uint8_t>& unm, bool* any_unm) {
  const char* const limit = "result deltas compare at most 4096 rules on either side";
  const size_t Rn = prog->p->rules.size();
  if (Rn > kpe_delta_max_rules()) return fail(KPE_E_LIMIT, limit);
  if (!c->d || c->d->kept_rules < 0) return fail(KPE_E_STATE, "no kept result on this corpus");
  const size_t Ro = (size_t)c->d->kept_rules;
  if (Ro > kpe_delta_max_rules()) return fail(KPE_E_LIMIT, limit);
  std::vector<int32_t> own;
  if (!old_of) {
    own.resize(std::max<size_t>(Rn, 1));
    if (kpe_status st = kpe_delta_column_map(c, prog, own.data())) return st;
    old_of = own.data();
  }
  if (kpe_status st = delta_map_check(old_of, Rn, Ro, unm)) return st;
  *any_unm = false;
  for (uint8_t& u : unm) {  // named -> unmapped
    u = u ? 0 : 1;
    *any_unm |= u != 0;
  }
  tab.resize(Rn);
  for (size_t r = 0; r < Rn; ++r)
    tab[r] = (old_of[r] < 0 ? 0xFFFFu : (uint32_t)old_of[r]) | ((uint32_t)(always ? always[r] : 0) << 16);
  return KPE_OK;
}
// the binding checks of a query on the new matrix (under dev->mu)
static kpe_status delta_bound(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c) {
  HIPCHK(hipSetDevice(dev->ordinal));
  if (c->d->bind.prog != prog->p.get()) return fail(KPE_E_STATE, "no evaluation of this program on this corpus");
  if (c->d->ordinal != dev->ordinal) return fail(KPE_E_STATE, "corpus not uploaded to this device");
  return KPE_OK;
}

static kpe_status changed_impl(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, const int32_t* old_of,
                               const uint8_t* always, uint64_t* rows_out, uint8_t* vrows_out, uint64_t cap,
                               uint64_t* total_out) {
  *total_out = 0;
  if (!dev || !prog || !c) return fail(KPE_E_INVALID, "null argument");
  if (cap && !rows_out) return fail(KPE_E_INVALID, "cap > 0 without a rows buffer");
  std::vector<uint32_t> tab;
  std::vector<uint8_t> unm;
  bool any_unm = false;
  if (kpe_status st = delta_tables(prog, c, old_of, always, tab, unm, &any_unm)) return st;
  const size_t Rn = tab.size(), Ro = unm.size();
  const uint64_t n = (uint64_t)c->c->n;
  std::lock_guard<std::mutex> lk(dev->mu);
  if (kpe_status st = delta_bound(dev, prog, c)) return st;
  if (!n) return KPE_OK;
  kpe::DeviceCorpus& D = *c->d;
  auto& B = D.bind;
  hipStream_t s = B.last ? B.last : dev->stream;
  // scratch of this call (freed on every return path): the row flags as an N x 1 matrix for the
  // selection chain, its tile offsets and counts, the tables
  const uint64_t ntiles = (n + 4095u) / 4096u;
  const size_t flag_bytes = (size_t)((n + 15u) & ~(uint64_t)15u);
  const size_t off_bytes = (size_t)((ntiles + 2) & ~(uint64_t)1) * 8;
  const size_t cnt_bytes = (size_t)((ntiles + 3) & ~(uint64_t)3) * 4;
  const size_t tab_bytes = (Rn * 4 + 15u) & ~(size_t)15u;
  DevBuf scratch, drows, dverd;
  HIPCHK(scratch.ensure(flag_bytes + off_bytes + cnt_bytes + tab_bytes + Ro + 16));
  uint8_t* base = scratch.as<uint8_t>();
  uint8_t* d_flags = base;
  uint64_t* d_off = reinterpret_cast<uint64_t*>(base + flag_bytes);
  uint32_t* d_cnt = reinterpret_cast<uint32_t*>(base + flag_bytes + off_bytes);
  uint32_t* d_tab = reinterpret_cast<uint32_t*>(base + flag_bytes + off_bytes + cnt_bytes);
  uint8_t* d_sel = base + flag_bytes + off_bytes + cnt_bytes + tab_bytes;  // the flag matrix's one mask
  uint8_t* d_unm = d_sel + 16;
  const uint8_t sel1 = (uint8_t)KPE_SEL(1);
  if (Rn) HIPCHK(hipMemcpyAsync(d_tab, tab.data(), Rn * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d_sel, &sel1, 1, hipMemcpyHostToDevice, s));
  if (any_unm) HIPCHK(hipMemcpyAsync(d_unm, unm.data(), Ro, hipMemcpyHostToDevice, s));
  HIPCHK(kpe_launch_delta_flags(B.verdicts.as<uint8_t>(), D.kept.as<uint8_t>(), n, (uint32_t)Rn, (uint32_t)Ro, d_tab,
                                any_unm ? d_unm : nullptr, d_flags, s));
  HIPCHK(kpe_launch_select_count(d_flags, n, 1u, d_sel, 0, d_cnt, d_off, s));
  uint64_t total = 0;
  HIPCHK(hipMemcpyAsync(&total, d_off + ntiles, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *total_out = total;
  const uint64_t m = std::min(total, cap);
  if (!m) return KPE_OK;
  HIPCHK(drows.ensure((size_t)m * 8));
  HIPCHK(kpe_launch_select_scatter(d_flags, n, 1u, d_sel, 0, d_off, m, drows.as<uint64_t>(), nullptr, s));
  const bool vr = vrows_out && Rn;
  if (vr) {
    HIPCHK(dverd.ensure((size_t)m * Rn));
    HIPCHK(kpe_launch_gather_rows(B.verdicts.as<uint8_t>(), (uint32_t)Rn, drows.as<uint64_t>(), m, dverd.as<uint8_t>(), s));
  }
  HIPCHK(hipMemcpyAsync(rows_out, drows.p, (size_t)m * 8, hipMemcpyDeviceToHost, s));
  if (vr) HIPCHK(hipMemcpyAsync(vrows_out, dverd.p, (size_t)m * Rn, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return KPE_OK;
}

int64_t kpe_changed_rows(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, const int32_t* old_of,
                         const uint8_t* always, uint64_t* rows, uint8_t* verdict_rows, uint64_t cap) {
  uint64_t total = 0;
  const kpe_status st = changed_impl(dev, prog, c, old_of, always, rows, verdict_rows, cap, &total);
  return st ? -(int64_t)st : (int64_t)total;
}

// What kpe_changed_pairs and kpe_changed_pairs_fp check of their pair list before any device call.
static kpe_status pairs_args(const kpe_device* dev, const kpe_program* prog, const kpe_corpus* c_new,
                             const kpe_corpus* c_old, const uint64_t* pairs, uint64_t npairs, const uint64_t* changed,
                             uint64_t cap) {
  if (!dev || !prog || !c_new || !c_old || (npairs && !pairs)) return fail(KPE_E_INVALID, "null argument");
  if (cap && !changed) return fail(KPE_E_INVALID, "cap > 0 without a changed buffer");
  const uint64_t nn = (uint64_t)c_new->c->n, no = (uint64_t)c_old->c->n;
  for (uint64_t k = 0; k < npairs; ++k)
    if (pairs[2 * k] >= nn || pairs[2 * k + 1] >= no) return fail(KPE_E_INVALID, "pair row past its corpus");
  return KPE_OK;
}
// Their state checks (under dev->mu), and the stream of the comparison: the one of c_new's last
// evaluation, after c_old's pending work (its keep is enqueued on its own stream).
static kpe_status pairs_bound(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c_new, const kpe_corpus* c_old,
                              hipStream_t* s) {
  if (!c_new->d) return fail(KPE_E_STATE, "corpus not uploaded");
  if (kpe_status st = delta_bound(dev, prog, c_new)) return st;
  if (c_old->d->ordinal != dev->ordinal) return fail(KPE_E_STATE, "corpus not uploaded to this device");
  *s = c_new->d->bind.last ? c_new->d->bind.last : dev->stream;
  const hipStream_t so = c_old->d->bind.last;
  if (so && so != *s) HIPCHK(hipStreamSynchronize(so));
  return KPE_OK;
}
// The carve of a pair call's scratch: the pairs, their flag bytes as an npairs x 1 matrix for the
// selection chain, its tile offsets and counts and its one mask, then `extra` bytes (16-byte aligned).
struct PairScratch {
  uint64_t ntiles;
  uint64_t* d_pairs;
  uint8_t* d_flags;
  uint64_t* d_off;
  uint32_t* d_cnt;
  uint8_t* d_sel;
  uint8_t* d_extra;
};
static kpe_status pairs_scratch(DevBuf& scratch, const uint64_t* pairs, uint64_t npairs, size_t extra, hipStream_t s,
                                PairScratch* o) {
  o->ntiles = (npairs + 4095u) / 4096u;
  const size_t pair_bytes = (size_t)npairs * 16;
  const size_t flag_bytes = (size_t)((npairs + 15u) & ~(uint64_t)15u);
  const size_t off_bytes = (size_t)((o->ntiles + 2) & ~(uint64_t)1) * 8;
  const size_t cnt_bytes = (size_t)((o->ntiles + 3) & ~(uint64_t)3) * 4;
  HIPCHK(scratch.ensure(pair_bytes + flag_bytes + off_bytes + cnt_bytes + 16 + extra));
  uint8_t* base = scratch.as<uint8_t>();
  o->d_pairs = reinterpret_cast<uint64_t*>(base);
  o->d_flags = base + pair_bytes;
  o->d_off = reinterpret_cast<uint64_t*>(base + pair_bytes + flag_bytes);
  o->d_cnt = reinterpret_cast<uint32_t*>(base + pair_bytes + flag_bytes + off_bytes);
  o->d_sel = base + pair_bytes + flag_bytes + off_bytes + cnt_bytes;
  o->d_extra = o->d_sel + 16;
  static const uint8_t sel1 = (uint8_t)KPE_SEL(1);
  HIPCHK(hipMemcpyAsync(o->d_pairs, pairs, pair_bytes, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(o->d_sel, &sel1, 1, hipMemcpyHostToDevice, s));
  return KPE_OK;
}

static kpe_status changed_pairs_impl(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c_new,
                                     const kpe_corpus* c_old, const uint64_t* pairs, uint64_t npairs,
                                     const int32_t* old_of, const uint8_t* always, uint64_t* changed_out,
                                     uint8_t* vrows_out, uint64_t cap, uint64_t* total_out) {
  *total_out = 0;
  if (kpe_status st = pairs_args(dev, prog, c_new, c_old, pairs, npairs, changed_out, cap)) return st;
  std::vector<uint32_t> tab;
  std::vector<uint8_t> unm;
  bool any_unm = false;
  if (kpe_status st = delta_tables(prog, c_old, old_of, always, tab, unm, &any_unm)) return st;
  const size_t Rn = tab.size(), Ro = unm.size();
  std::lock_guard<std::mutex> lk(dev->mu);
  hipStream_t s = nullptr;
  if (kpe_status st = pairs_bound(dev, prog, c_new, c_old, &s)) return st;
  if (!npairs) return KPE_OK;
  const uint8_t* vnew = c_new->d->bind.verdicts.as<uint8_t>();
  const size_t tab_bytes = (Rn * 4 + 15u) & ~(size_t)15u;
  DevBuf scratch, didx, drows, dverd;  // this call's, freed on every return path
  PairScratch S;
  if (kpe_status st = pairs_scratch(scratch, pairs, npairs, tab_bytes + Ro, s, &S)) return st;
  uint32_t* d_tab = reinterpret_cast<uint32_t*>(S.d_extra);
  uint8_t* d_unm = S.d_extra + tab_bytes;
  if (Rn) HIPCHK(hipMemcpyAsync(d_tab, tab.data(), Rn * 4, hipMemcpyHostToDevice, s));
  if (any_unm) HIPCHK(hipMemcpyAsync(d_unm, unm.data(), Ro, hipMemcpyHostToDevice, s));
  HIPCHK(kpe_launch_delta_pairs(vnew, c_old->d->kept.as<uint8_t>(), S.d_pairs, npairs, (uint32_t)Rn, (uint32_t)Ro, d_tab,
                                any_unm ? d_unm : nullptr, S.d_flags, s));
  HIPCHK(kpe_launch_select_count(S.d_flags, npairs, 1u, S.d_sel, 0, S.d_cnt, S.d_off, s));
  uint64_t total = 0;
  HIPCHK(hipMemcpyAsync(&total, S.d_off + S.ntiles, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));  // also: pairs and the tables are copied
  *total_out = total;
  const uint64_t m = std::min(total, cap);
  if (!m) return KPE_OK;
  HIPCHK(didx.ensure((size_t)m * 8));
  HIPCHK(kpe_launch_select_scatter(S.d_flags, npairs, 1u, S.d_sel, 0, S.d_off, m, didx.as<uint64_t>(), nullptr, s));
  const bool vr = vrows_out && Rn;
  if (vr) {
    HIPCHK(drows.ensure((size_t)m * 8));
    HIPCHK(dverd.ensure((size_t)m * Rn));
    HIPCHK(kpe_launch_pair_rows(S.d_pairs, didx.as<uint64_t>(), m, drows.as<uint64_t>(), s));
    HIPCHK(kpe_launch_gather_rows(vnew, (uint32_t)Rn, drows.as<uint64_t>(), m, dverd.as<uint8_t>(), s));
  }
  HIPCHK(hipMemcpyAsync(changed_out, didx.p, (size_t)m * 8, hipMemcpyDeviceToHost, s));
  if (vr) HIPCHK(hipMemcpyAsync(vrows_out, dverd.p, (size_t)m * Rn, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return KPE_OK;
}

int64_t kpe_changed_pairs(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c_new, const kpe_corpus* c_old,
                          const uint64_t* pairs, uint64_t npairs, const int32_t* old_of, const uint8_t* always,
                          uint64_t* changed, uint8_t* verdict_rows, uint64_t cap) {
  uint64_t total = 0;
  const kpe_status st =
      changed_pairs_impl(dev, prog, c_new, c_old, pairs, npairs, old_of, always, changed, verdict_rows, cap, &total);
  return st ? -(int64_t)st : (int64_t)total;
}

kpe_status kpe_delta_transitions(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, const int32_t* old_of,
                                 uint64_t* out) {
  if (!dev || !prog || !c) return fail(KPE_E_INVALID, "null argument");
  if (!out && prog->p->rules.size()) return fail(KPE_E_INVALID, "null argument");
  std::vector<uint32_t> tab;
  std::vector<uint8_t> unm;
  bool any_unm = false;
  if (kpe_status st = delta_tables(prog, c, old_of, nullptr, tab, unm, &any_unm)) return st;
  const size_t Rn = tab.size(), Ro = unm.size();
  std::lock_guard<std::mutex> lk(dev->mu);
  if (kpe_status st = delta_bound(dev, prog, c)) return st;
  if (!Rn) return KPE_OK;
  kpe::DeviceCorpus& D = *c->d;
  auto& B = D.bind;
  hipStream_t s = B.last ? B.last : dev->stream;
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit counters");
  const size_t out_bytes = Rn * 64 * sizeof(uint64_t);
  DevBuf scratch;  // this call's: the tables' counters, then the map
  HIPCHK(scratch.ensure(out_bytes + Rn * 4));
  uint32_t* d_tab = reinterpret_cast<uint32_t*>(scratch.as<uint8_t>() + out_bytes);
  HIPCHK(hipMemcpyAsync(d_tab, tab.data(), Rn * 4, hipMemcpyHostToDevice, s));
  HIPCHK(kpe_launch_delta_transitions(B.verdicts.as<uint8_t>(), D.kept.as<uint8_t>(), (uint64_t)c->c->n, (uint32_t)Rn,
                                      (uint32_t)Ro, d_tab, scratch.as<unsigned long long>(), s));
  HIPCHK(hipMemcpyAsync(out, scratch.p, out_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return KPE_OK;
}

// ---- policy edits on a kept result: the plan, the splice, its changed rows ---------------------
namespace {
std::string splice_policy_of(const std::string& name) { return name.substr(0, name.find('/')); }

// The column plan of include/kpe.h over two name lists, and the partner (the kept column of the
// same name, or -1) of every column of sub.
kpe_status splice_plan_build(const std::vector<std::string>& kept, const std::vector<std::string>& sub,
                             const char* const* removed, uint32_t nremoved, std::vector<int32_t>& plan,
                             std::vector<int32_t>& partner) {
  std::map<std::string, int32_t> kept_col, sub_col;
  for (size_t r = 0; r < kept.size(); ++r)
    if (!kept_col.emplace(kept[r], (int32_t)r).second) return fail(KPE_E_INVALID, "kept rule name occurs twice: " + kept[r]);
  std::map<std::string, std::vector<int32_t>> by_policy;  // policy of sub -> its columns, in sub's order
  std::vector<std::string> order;                         // sub's policies, by first column
  for (size_t s = 0; s < sub.size(); ++s) {
    if (!sub_col.emplace(sub[s], (int32_t)s).second) return fail(KPE_E_INVALID, "rule name occurs twice: " + sub[s]);
    auto& cols = by_policy[splice_policy_of(sub[s])];
    if (cols.empty()) order.push_back(splice_policy_of(sub[s]));
    cols.push_back((int32_t)s);
  }
  std::map<std::string, bool> gone;
  for (uint32_t k = 0; k < nremoved; ++k) {
    if (!removed || !removed[k]) return fail(KPE_E_INVALID, "null argument");
    if (by_policy.count(removed[k])) return fail(KPE_E_INVALID, std::string("removed policy is also edited: ") + removed[k]);
    gone[removed[k]] = true;
  }
  plan.clear();
  std::map<std::string, bool> emitted;
  const auto emit = [&](const std::string& pol) {
    for (int32_t s : by_policy[pol]) plan.push_back(-1 - s);
    emitted[pol] = true;
  };
  for (size_t c = 0; c < kept.size(); ++c) {
    const std::string pol = splice_policy_of(kept[c]);
    if (by_policy.count(pol)) {
      if (!emitted.count(pol)) emit(pol);  // an edited policy keeps its place
    } else if (!gone.count(pol)) {
      plan.push_back((int32_t)c);
    }
  }
  for (const std::string& pol : order)
    if (!emitted.count(pol)) emit(pol);  // added policies, at the end
  partner.resize(sub.size());
  for (size_t s = 0; s < sub.size(); ++s) {
    const auto it = kept_col.find(sub[s]);
    partner[s] = it == kept_col.end() ? -1 : it->second;
  }
  return KPE_OK;
}

const char* const kSpliceLimit = "a splice takes at most 4096 rules on any side";
kpe_status splice_limit(size_t Ro, size_t Rs, size_t rn) {
  if (Ro > KPE_DELTA_MAX_RULES || Rs > KPE_DELTA_MAX_RULES || rn > KPE_DELTA_MAX_RULES) return fail(KPE_E_LIMIT, kSpliceLimit);
  return KPE_OK;
}
std::vector<std::string> program_names(const kpe::Program& P) {
  std::vector<std::string> names(P.rule_names.begin(), P.rule_names.end());
  names.resize(P.rules.size());
  return names;
}

// What the host twin and the device call check of a plan, and the tables the kernel reads (col,
// unm: kernels_launch.h kpe_launch_splice).
kpe_status splice_tables(const int32_t* plan, size_t rn, const int32_t* partner, size_t Rs, size_t Ro,
                         const uint8_t* always, std::vector<uint32_t>& col, std::vector<uint8_t>& unm, bool* any_unm) {
  std::vector<uint8_t> copied(Ro, 0), emitted(Rs, 0);
  col.assign(2 * rn, 0);
  unm.assign(Ro, 1);
  for (size_t s = 0; s < Rs; ++s) {
    const int32_t p = partner[s];
    if (p == -1) continue;
    if (p < -1 || (size_t)p >= Ro) return fail(KPE_E_INVALID, "partner outside the kept rules");
    if (!unm[(size_t)p]) return fail(KPE_E_INVALID, "partner names a kept column twice");
    unm[(size_t)p] = 0;
  }
  for (size_t r = 0; r < rn; ++r) {
    const int32_t e = plan[r];
    if (e >= 0) {
      if ((size_t)e >= Ro) return fail(KPE_E_INVALID, "plan entry outside the kept rules");
      if (copied[(size_t)e]) return fail(KPE_E_INVALID, "plan copies a kept column twice");
      if (!unm[(size_t)e]) return fail(KPE_E_INVALID, "plan copies a partner column");
      copied[(size_t)e] = 1;
      col[2 * r] = (uint32_t)e;
    } else {
      const size_t s = (size_t)(-1 - (int64_t)e);
      if (s >= Rs) return fail(KPE_E_INVALID, "plan entry outside the sub rules");
      if (emitted[s]) return fail(KPE_E_INVALID, "plan emits a sub column twice");
      emitted[s] = 1;
      col[2 * r] = 0x80000000u | (uint32_t)s;
      col[2 * r + 1] = (partner[s] < 0 ? 0xFFFFu : (uint32_t)partner[s]) | ((uint32_t)(always ? always[s] : 0) << 16);
    }
  }
  for (size_t s = 0; s < Rs; ++s)
    if (!emitted[s]) return fail(KPE_E_INVALID, "plan leaves a sub column out");
  *any_unm = false;
  for (size_t o = 0; o < Ro; ++o) {
    if (copied[o]) unm[o] = 0;
    *any_unm |= unm[o] != 0;
  }
  return KPE_OK;
}
}  // namespace

int64_t kpe_splice_plan_names(const char* const* kept, uint32_t Ro, const char* const* sub, uint32_t Rs,
                              const char* const* removed, uint32_t nremoved, int32_t* plan, int32_t* partner,
                              uint32_t cap) {
  if ((Ro && !kept) || (Rs && !sub) || (cap && !plan)) return -(int64_t)fail(KPE_E_INVALID, "null argument");
  std::vector<std::string> kn(Ro), sn(Rs);
  for (uint32_t r = 0; r < Ro; ++r) {
    if (!kept[r]) return -(int64_t)fail(KPE_E_INVALID, "null argument");
    kn[r] = kept[r];
  }
  for (uint32_t s = 0; s < Rs; ++s) {
    if (!sub[s]) return -(int64_t)fail(KPE_E_INVALID, "null argument");
    sn[s] = sub[s];
  }
  std::vector<int32_t> pl, pa;
  if (kpe_status st = splice_plan_build(kn, sn, removed, nremoved, pl, pa)) return -(int64_t)st;
  for (size_t r = 0; r < pl.size() && r < cap; ++r) plan[r] = pl[r];
  if (partner)
    for (uint32_t s = 0; s < Rs; ++s) partner[s] = pa[s];
  return (int64_t)pl.size();
}

int64_t kpe_splice_plan(const kpe_corpus* c, const kpe_program* sub, const char* const* removed, uint32_t nremoved,
                        int32_t* plan, uint32_t cap) {
  if (!c || !sub || (cap && !plan)) return -(int64_t)fail(KPE_E_INVALID, "null argument");
  if (!c->d || c->d->kept_rules < 0) return -(int64_t)fail(KPE_E_STATE, "no kept result on this corpus");
  std::vector<int32_t> pl, pa;
  if (kpe_status st = splice_plan_build(c->d->kept_names, program_names(*sub->p), removed, nremoved, pl, pa))
    return -(int64_t)st;
  if (kpe_status st = splice_limit(c->d->kept_names.size(), pa.size(), pl.size())) return -(int64_t)st;
  for (size_t r = 0; r < pl.size() && r < cap; ++r) plan[r] = pl[r];
  return (int64_t)pl.size();
}

int64_t kpe_results_splice_host(const uint8_t* kept, const uint8_t* sub_v, uint64_t n, uint32_t Ro, uint32_t Rs,
                                uint32_t rn, const int32_t* plan, const int32_t* partner, const uint8_t* always,
                                uint8_t* out, uint8_t* flags) {
  if ((rn && !plan) || (Rs && !partner)) return -(int64_t)fail(KPE_E_INVALID, "null argument");
  if (n && ((Ro && !kept) || (Rs && !sub_v) || (rn && !out) || !flags)) return -(int64_t)fail(KPE_E_INVALID, "null argument");
  std::vector<uint32_t> col;
  std::vector<uint8_t> unm;
  bool any_unm = false;
  if (kpe_status st = splice_tables(plan, rn, partner, Rs, Ro, always, col, unm, &any_unm)) return -(int64_t)st;
  uint64_t total = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t* k = kept + (size_t)i * Ro;
    const uint8_t* e = sub_v + (size_t)i * Rs;
    uint8_t* o = out + (size_t)i * rn;
    for (uint32_t r = 0; r < rn; ++r) o[r] = plan[r] >= 0 ? k[plan[r]] : e[-1 - plan[r]];
    bool ch = false;
    for (uint32_t s = 0; s < Rs && !ch; ++s) {
      const uint8_t x = e[s], p = partner[s] >= 0 ? k[partner[s]] : (uint8_t)KPE_NA;
      ch = x != p || delta_always(always, s, x);
    }
    for (uint32_t c = 0; c < Ro && !ch && any_unm; ++c) ch = unm[c] && k[c] != KPE_NA;
    flags[i] = ch ? 1 : 0;
    total += ch;
  }
  return (int64_t)total;
}

double kpe_splice_bytes(uint64_t n, uint32_t Ro, uint32_t Rs, uint32_t rn) {
  return (double)n * ((double)Ro + (double)Rs + (double)rn + 1.0);
}
uint32_t kpe_splice_group_rows(uint32_t Ro, uint32_t Rs, uint32_t rn) { return kpe_splice_rows_per_group(Ro, Rs, rn); }
uint32_t kpe_splice_max_groups(void) { return kpe_splice_grid(); }

static kpe_status splice_impl(kpe_device* dev, const kpe_program* sub, kpe_corpus* c, const char* const* removed,
                              uint32_t nremoved, const uint8_t* always, uint64_t* total_out) {
  *total_out = 0;
  if (!dev || !sub || !c) return fail(KPE_E_INVALID, "null argument");
  if (!c->d || c->d->kept_rules < 0) return fail(KPE_E_STATE, "no kept result on this corpus");
  kpe::DeviceCorpus& D = *c->d;
  const std::vector<std::string> sub_names = program_names(*sub->p);
  std::vector<int32_t> plan, partner;
  if (kpe_status st = splice_plan_build(D.kept_names, sub_names, removed, nremoved, plan, partner)) return st;
  const size_t Ro = (size_t)D.kept_rules, Rs = sub_names.size(), rn = plan.size();
  if (kpe_status st = splice_limit(Ro, Rs, rn)) return st;
  std::vector<uint32_t> col;
  std::vector<uint8_t> unm;
  bool any_unm = false;
  if (kpe_status st = splice_tables(plan.data(), rn, partner.data(), Rs, Ro, always, col, unm, &any_unm)) return st;
  std::vector<std::string> names(rn);
  for (size_t r = 0; r < rn; ++r) names[r] = plan[r] >= 0 ? D.kept_names[(size_t)plan[r]] : sub_names[(size_t)(-1 - plan[r])];
  const uint64_t n = (uint64_t)c->c->n;
  std::lock_guard<std::mutex> lk(dev->mu);
  if (Rs) {
    if (kpe_status st = delta_bound(dev, sub, c)) return st;
  } else {  // only removals: there is no E to read, so no evaluation of sub is asked for
    HIPCHK(hipSetDevice(dev->ordinal));
    if (D.ordinal != dev->ordinal) return fail(KPE_E_STATE, "corpus not uploaded to this device");
  }
  auto& B = D.bind;
  // on the stream of the evaluation of sub: after it, and before the corpus's next one
  hipStream_t s = B.last ? B.last : dev->stream;
  D.splice_valid = false;
  uint64_t total = 0;
  if (n) {
    const uint64_t ntiles = (n + 4095u) / 4096u;
    const size_t off_bytes = (size_t)((ntiles + 2) & ~(uint64_t)1) * 8;
    const size_t cnt_bytes = (size_t)((ntiles + 3) & ~(uint64_t)3) * 4;
    const size_t col_bytes = (col.size() * 4 + 15u) & ~(size_t)15u;
    DevBuf scratch;  // this call's, freed on every return path: the selection's tiles, its mask, the tables
    HIPCHK(scratch.ensure(off_bytes + cnt_bytes + col_bytes + 16 + Ro));
    HIPCHK(D.kept_spare.ensure(n * std::max<size_t>(rn, 1)));
    HIPCHK(D.splice_flags.ensure((size_t)((n + 15u) & ~(uint64_t)15u)));
    uint8_t* base = scratch.as<uint8_t>();
    uint64_t* d_off = reinterpret_cast<uint64_t*>(base);
    uint32_t* d_cnt = reinterpret_cast<uint32_t*>(base + off_bytes);
    uint32_t* d_col = reinterpret_cast<uint32_t*>(base + off_bytes + cnt_bytes);
    uint8_t* d_sel = base + off_bytes + cnt_bytes + col_bytes;
    uint8_t* d_unm = d_sel + 16;
    const uint8_t sel1 = (uint8_t)KPE_SEL(1);
    if (rn) HIPCHK(hipMemcpyAsync(d_col, col.data(), col.size() * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_sel, &sel1, 1, hipMemcpyHostToDevice, s));
    if (any_unm) HIPCHK(hipMemcpyAsync(d_unm, unm.data(), Ro, hipMemcpyHostToDevice, s));
    HIPCHK(kpe_launch_splice(D.kept.as<uint8_t>(), B.verdicts.as<uint8_t>(), n, (uint32_t)Ro, (uint32_t)Rs, (uint32_t)rn,
                             d_col, any_unm ? d_unm : nullptr, D.kept_spare.as<uint8_t>(), D.splice_flags.as<uint8_t>(), s));
    HIPCHK(kpe_launch_select_count(D.splice_flags.as<uint8_t>(), n, 1u, d_sel, 0, d_cnt, d_off, s));
    HIPCHK(hipMemcpyAsync(&total, d_off + ntiles, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::swap(D.kept.p, D.kept_spare.p);
    std::swap(D.kept.bytes, D.kept_spare.bytes);
  }
  D.kept_names.swap(names);
  D.kept_rules = (int64_t)rn;
  D.splice_valid = true;
  *total_out = total;
  return KPE_OK;
}

int64_t kpe_results_splice(kpe_device* dev, const kpe_program* sub, kpe_corpus* c, const char* const* removed,
                           uint32_t nremoved, const uint8_t* always) {
  uint64_t total = 0;
  const kpe_status st = splice_impl(dev, sub, c, removed, nremoved, always, &total);
  return st ? -(int64_t)st : (int64_t)total;
}

static kpe_status spliced_impl(kpe_device* dev, const kpe_corpus* c, uint64_t* rows_out, uint8_t* vrows_out, uint64_t cap,
                               uint64_t* total_out) {
  *total_out = 0;
  if (!dev || !c) return fail(KPE_E_INVALID, "null argument");
  if (cap && !rows_out) return fail(KPE_E_INVALID, "cap > 0 without a rows buffer");
  if (!c->d || c->d->kept_rules < 0 || !c->d->splice_valid) return fail(KPE_E_STATE, "no splice on this corpus");
  std::lock_guard<std::mutex> lk(dev->mu);
  HIPCHK(hipSetDevice(dev->ordinal));
  kpe::DeviceCorpus& D = *c->d;
  if (D.ordinal != dev->ordinal) return fail(KPE_E_STATE, "corpus not uploaded to this device");
  const uint64_t n = (uint64_t)c->c->n;
  const size_t rn = (size_t)D.kept_rules;
  if (!n) return KPE_OK;
  hipStream_t s = D.bind.last ? D.bind.last : dev->stream;
  const uint64_t ntiles = (n + 4095u) / 4096u;
  const size_t off_bytes = (size_t)((ntiles + 2) & ~(uint64_t)1) * 8;
  const size_t cnt_bytes = (size_t)((ntiles + 3) & ~(uint64_t)3) * 4;
  DevBuf scratch, drows, dverd;
  HIPCHK(scratch.ensure(off_bytes + cnt_bytes + 16));
  uint8_t* base = scratch.as<uint8_t>();
  uint64_t* d_off = reinterpret_cast<uint64_t*>(base);
  uint32_t* d_cnt = reinterpret_cast<uint32_t*>(base + off_bytes);
  uint8_t* d_sel = base + off_bytes + cnt_bytes;
  const uint8_t* d_flags = D.splice_flags.as<uint8_t>();
  const uint8_t sel1 = (uint8_t)KPE_SEL(1);
  HIPCHK(hipMemcpyAsync(d_sel, &sel1, 1, hipMemcpyHostToDevice, s));
  HIPCHK(kpe_launch_select_count(d_flags, n, 1u, d_sel, 0, d_cnt, d_off, s));
  uint64_t total = 0;
  HIPCHK(hipMemcpyAsync(&total, d_off + ntiles, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *total_out = total;
  const uint64_t m = std::min(total, cap);
  if (!m) return KPE_OK;
  HIPCHK(drows.ensure((size_t)m * 8));
  HIPCHK(kpe_launch_select_scatter(d_flags, n, 1u, d_sel, 0, d_off, m, drows.as<uint64_t>(), nullptr, s));
  const bool vr = vrows_out && rn;
  if (vr) {
    HIPCHK(dverd.ensure((size_t)m * rn));
    HIPCHK(kpe_launch_gather_rows(D.kept.as<uint8_t>(), (uint32_t)rn, drows.as<uint64_t>(), m, dverd.as<uint8_t>(), s));
  }
  HIPCHK(hipMemcpyAsync(rows_out, drows.p, (size_t)m * 8, hipMemcpyDeviceToHost, s));
  if (vr) HIPCHK(hipMemcpyAsync(vrows_out, dverd.p, (size_t)m * rn, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return KPE_OK;
}

int64_t kpe_spliced_rows(kpe_device* dev, const kpe_corpus* c, uint64_t* rows, uint8_t* verdict_rows, uint64_t cap) {
  uint64_t total = 0;
  const kpe_status st = spliced_impl(dev, c, rows, verdict_rows, cap, &total);
  return st ? -(int64_t)st : (int64_t)total;
}

kpe_status kpe_results_kept_fetch(kpe_device* dev, const kpe_corpus* c, uint64_t row0, uint64_t nrows, uint8_t* out) {
  if (!dev || !c) return fail(KPE_E_INVALID, "null argument");
  if (!c->d || c->d->kept_rules < 0) return fail(KPE_E_STATE, "no kept result on this corpus");
  const uint64_t n = (uint64_t)c->c->n;
  if (row0 > n || nrows > n - row0) return fail(KPE_E_INVALID, "rows past the corpus");
  const size_t R = (size_t)c->d->kept_rules;
  if (!nrows || !R) return KPE_OK;
  if (!out) return fail(KPE_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(dev->mu);
  HIPCHK(hipSetDevice(dev->ordinal));
  const kpe::DeviceCorpus& D = *c->d;
  if (D.ordinal != dev->ordinal) return fail(KPE_E_STATE, "corpus not uploaded to this device");
  hipStream_t s = D.bind.last ? D.bind.last : dev->stream;  // behind a pending keep
  HIPCHK(hipMemcpyAsync(out, D.kept.as<uint8_t>() + (size_t)row0 * R, (size_t)nrows * R, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return KPE_OK;
}

// ---- row fingerprints: 8 bytes per row, kept per corpus, compared on the device -----------------
static inline uint64_t fp_mix64(uint64_t z) {  // the splitmix64 finaliser
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

kpe_status kpe_fp_rule_salts(const kpe_program* prog, uint64_t* salts) {
  if (!prog) return fail(KPE_E_INVALID, "null argument");
  const kpe::Program& P = *prog->p;
  const size_t R = P.rules.size();
  if (R && !salts) return fail(KPE_E_INVALID, "null argument");
  for (size_t r = 0; r < R; ++r) {
    uint64_t h = 0xCBF29CE484222325ull;  // FNV-1a-64 of "<policy>/<rule>"
    if (r < P.rule_names.size())
      for (const unsigned char ch : P.rule_names[r]) h = (h ^ ch) * 0x100000001B3ull;
    h = fp_mix64(h);
    salts[r] = h ? h : 1;
  }
  return KPE_OK;
}

kpe_status kpe_row_fingerprints_host(uint32_t R, const uint8_t* verdicts, const uint32_t* cv_masks, uint64_t nrows,
                                     const uint64_t* salts, const uint64_t* msg_salts, uint8_t msg_codes,
                                     uint32_t flags, uint64_t* out) {
  if (flags & ~KPE_FP_MASKS) return fail(KPE_E_INVALID, "unknown fingerprint flag");
  if (nrows && !out) return fail(KPE_E_INVALID, "null argument");
  const bool with_masks = (flags & KPE_FP_MASKS) != 0;
  if (nrows && R && (!verdicts || !salts || (with_masks && !cv_masks))) return fail(KPE_E_INVALID, "null argument");
  if (!msg_salts) msg_salts = salts;
  for (uint64_t i = 0; i < nrows; ++i) {
    uint64_t fp = 0;
    for (uint32_t r = 0; r < R; ++r) {
      const uint8_t v = verdicts[(size_t)i * R + r];
      if (v == KPE_NA) continue;
      const uint64_t s = v < 8 && ((msg_codes >> v) & 1) ? msg_salts[r] : salts[r];
      const uint64_t m = with_masks && v == KPE_FAIL ? cv_masks[(size_t)i * R + r] : 0;
      fp += fp_mix64(s + 0x9E3779B97F4A7C15ull * ((uint64_t)v | (m << 8)));
    }
    out[i] = fp;
  }
  return KPE_OK;
}

int64_t kpe_changed_fingerprints_host(const uint64_t* old_fp, const uint64_t* new_fp, uint64_t n, uint64_t* rows,
                                      uint64_t cap) {
  if (cap && !rows) return -(int64_t)fail(KPE_E_INVALID, "cap > 0 without a rows buffer");
  if (n && (!old_fp || !new_fp)) return -(int64_t)fail(KPE_E_INVALID, "null argument");
  uint64_t total = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (old_fp[i] == new_fp[i]) continue;
    if (total < cap) rows[total] = i;
    ++total;
  }
  return (int64_t)total;
}

// What the device calls check before any device call, and the table the kernel reads:
// [salts: R][msg_salts: R].
static kpe_status fp_table(const kpe_program* prog, const uint64_t* salts, const uint64_t* msg_salts, uint32_t flags,
                           std::vector<uint64_t>& tbl) {
  if (flags & ~KPE_FP_MASKS) return fail(KPE_E_INVALID, "unknown fingerprint flag");
  const size_t R = prog->p->rules.size();
  if (R > kpe_delta_max_rules()) return fail(KPE_E_LIMIT, "row fingerprints take at most 4096 rules");
  tbl.resize(2 * R);
  if (!R) return KPE_OK;
  if (salts) memcpy(tbl.data(), salts, R * 8);
  else if (kpe_status st = kpe_fp_rule_salts(prog, tbl.data())) return st;
  memcpy(tbl.data() + R, msg_salts ? msg_salts : tbl.data(), R * 8);
  return KPE_OK;
}
// The binding checks of a fingerprint query (under dev->mu), and the launch: rows [row0, row0 +
// nrows) into d_out, the table copied from h_tbl (which must live until the copy ran) to d_tbl.
static kpe_status fp_compute(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, const uint64_t* h_tbl,
                             uint8_t msg_codes, uint32_t flags, uint64_t row0, uint64_t nrows, uint64_t* d_tbl,
                             uint64_t* d_out, hipStream_t s) {
  const size_t R = prog->p->rules.size();
  if (!nrows) return KPE_OK;
  if (!R) {
    HIPCHK(hipMemsetAsync(d_out, 0, (size_t)nrows * 8, s));
    return KPE_OK;
  }
  auto& B = c->d->bind;
  const uint32_t* d_masks = (flags & KPE_FP_MASKS) ? B.masks.as<uint32_t>() : nullptr;
  HIPCHK(hipMemcpyAsync(d_tbl, h_tbl, R * 16, hipMemcpyHostToDevice, s));
  HIPCHK(kpe_launch_row_fp(B.verdicts.as<uint8_t>(), d_masks, (uint32_t)R, row0, nrows, d_tbl, msg_codes, d_out, s));
  return KPE_OK;
}
static kpe_status fp_bound(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, uint32_t flags) {
  if (!c->d) return fail(KPE_E_STATE, "corpus not uploaded");
  if (kpe_status st = delta_bound(dev, prog, c)) return st;
  // the kernel reads a word per FAIL cell: the buffer must hold this program's N x R words
  const size_t cells = (size_t)c->c->n * prog->p->rules.size();
  if ((flags & KPE_FP_MASKS) && (!c->d->has_masks || c->d->bind.masks.bytes < cells * 4))
    return fail(KPE_E_STATE, "check masks were not computed");
  return KPE_OK;
}

kpe_status kpe_fetch_row_fingerprints(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c,
                                      const uint64_t* salts, const uint64_t* msg_salts, uint8_t msg_codes,
                                      uint32_t flags, uint64_t row0, uint64_t nrows, uint64_t* out) {
  if (!dev || !prog || !c || (nrows && !out)) return fail(KPE_E_INVALID, "null argument");
  std::vector<uint64_t> tbl;
  if (kpe_status st = fp_table(prog, salts, msg_salts, flags, tbl)) return st;
  if (row0 > (uint64_t)c->c->n || nrows > (uint64_t)c->c->n - row0) return fail(KPE_E_INVALID, "rows past the corpus");
  if (!nrows) return KPE_OK;
  const size_t R = tbl.size() / 2;
  if (!R) {
    memset(out, 0, nrows * 8);
    return KPE_OK;
  }
  if (!c->d) return fail(KPE_E_STATE, "corpus not uploaded");
  std::lock_guard<std::mutex> lk(dev->mu);
  if (kpe_status st = fp_bound(dev, prog, c, flags)) return st;
  auto& B = c->d->bind;
  hipStream_t s = B.last ? B.last : dev->stream;
  const size_t out_bytes = (size_t)nrows * 8;
  DevBuf scratch;  // this call's: the rows' fingerprints, then the table
  HIPCHK(scratch.ensure(out_bytes + R * 16));
  uint64_t* d_tbl = scratch.as<uint64_t>() + nrows;
  if (kpe_status st = fp_compute(dev, prog, c, tbl.data(), msg_codes, flags, row0, nrows, d_tbl, scratch.as<uint64_t>(), s))
    return st;
  HIPCHK(hipMemcpyAsync(out, scratch.p, out_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return KPE_OK;
}

kpe_status kpe_fingerprints_keep(kpe_device* dev, const kpe_program* prog, kpe_corpus* c, const uint64_t* salts,
                                 const uint64_t* msg_salts, uint8_t msg_codes, uint32_t flags) {
  if (!dev || !prog || !c) return fail(KPE_E_INVALID, "null argument");
  std::vector<uint64_t> tbl;
  if (kpe_status st = fp_table(prog, salts, msg_salts, flags, tbl)) return st;
  if (!c->d) return fail(KPE_E_STATE, "corpus not uploaded");
  std::lock_guard<std::mutex> lk(dev->mu);
  if (kpe_status st = fp_bound(dev, prog, c, flags)) return st;
  kpe::DeviceCorpus& D = *c->d;
  const uint64_t n = (uint64_t)c->c->n;
  const size_t R = tbl.size() / 2;
  D.fps_kept = false;
  HIPCHK(D.fps.ensure((size_t)n * 8 + R * 16));  // the fingerprints, then the table
  // the table's copy is enqueued, not waited for: its host bytes belong to the corpus
  D.fps_tbl.swap(tbl);
  hipStream_t s = D.bind.last ? D.bind.last : dev->stream;
  if (kpe_status st = fp_compute(dev, prog, c, D.fps_tbl.data(), msg_codes, flags, 0, n, D.fps.as<uint64_t>() + n,
                                 D.fps.as<uint64_t>(), s))
    return st;
  D.fps_kept = true;
  return KPE_OK;
}

kpe_status kpe_fingerprints_load(kpe_device* dev, kpe_corpus* c, const uint64_t* fp, uint64_t n) {
  if (!dev || !c || (n && !fp)) return fail(KPE_E_INVALID, "null argument");
  if (n != (uint64_t)c->c->n) return fail(KPE_E_INVALID, "one fingerprint per row of the corpus");
  if (!c->d) return fail(KPE_E_STATE, "corpus not uploaded");
  std::lock_guard<std::mutex> lk(dev->mu);
  HIPCHK(hipSetDevice(dev->ordinal));
  kpe::DeviceCorpus& D = *c->d;
  if (D.ordinal != dev->ordinal) return fail(KPE_E_STATE, "corpus not uploaded to this device");
  D.fps_kept = false;
  HIPCHK(D.fps.ensure((size_t)n * 8));
  hipStream_t s = D.bind.last ? D.bind.last : dev->stream;
  if (n) {
    HIPCHK(hipMemcpyAsync(D.fps.p, fp, (size_t)n * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));  // fp is the caller's
  }
  D.fps_kept = true;
  return KPE_OK;
}

kpe_status kpe_fingerprints_fetch(kpe_device* dev, const kpe_corpus* c, uint64_t row0, uint64_t nrows, uint64_t* out) {
  if (!dev || !c || (nrows && !out)) return fail(KPE_E_INVALID, "null argument");
  if (row0 > (uint64_t)c->c->n || nrows > (uint64_t)c->c->n - row0) return fail(KPE_E_INVALID, "rows past the corpus");
  if (!c->d || !c->d->fps_kept) return fail(KPE_E_STATE, "no kept fingerprints on this corpus");
  if (!nrows) return KPE_OK;
  std::lock_guard<std::mutex> lk(dev->mu);
  HIPCHK(hipSetDevice(dev->ordinal));
  const kpe::DeviceCorpus& D = *c->d;
  if (D.ordinal != dev->ordinal) return fail(KPE_E_STATE, "corpus not uploaded to this device");
  hipStream_t s = D.bind.last ? D.bind.last : dev->stream;
  HIPCHK(hipMemcpyAsync(out, D.fps.as<uint64_t>() + row0, (size_t)nrows * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return KPE_OK;
}

kpe_status kpe_fingerprints_drop(kpe_device* dev, kpe_corpus* c) {
  if (!dev || !c) return fail(KPE_E_INVALID, "null argument");
  if (!c->d) return KPE_OK;
  std::lock_guard<std::mutex> lk(dev->mu);
  HIPCHK(hipSetDevice(dev->ordinal));
  kpe::DeviceCorpus& D = *c->d;
  D.fps_kept = false;
  if (D.fps.p) HIPCHK(hipFree(D.fps.p));  // waits for a pending keep
  D.fps.p = nullptr, D.fps.bytes = 0;
  return KPE_OK;
}

int kpe_fingerprints_kept(const kpe_corpus* c) { return c && c->d && c->d->fps_kept ? 1 : 0; }

// ---- kept results carried into a gathered corpus ------------------------------------------------
kpe_status kpe_results_gather(kpe_device* dev, kpe_corpus* dst, const kpe_corpus* const* srcs, int nsrcs,
                              const uint64_t* pairs, uint64_t npairs, uint32_t what) {
  if (!dev || !dst) return fail(KPE_E_INVALID, "kpe_results_gather: null argument");
  if (what & ~(KPE_GATHER_MATRIX | KPE_GATHER_FINGERPRINTS)) return fail(KPE_E_INVALID, "kpe_results_gather: unknown flag");
  std::vector<uint8_t> listed;
  if (kpe_status st = kpe::gather_args("kpe_results_gather", srcs, nsrcs, pairs, npairs, &listed)) return st;
  if (npairs != (uint64_t)dst->c->n) return fail(KPE_E_INVALID, "kpe_results_gather: one pair per row of dst");
  for (int t = 0; t < nsrcs; ++t)
    if (srcs[t] == dst) return fail(KPE_E_INVALID, "kpe_results_gather: dst is among the sources");
  std::lock_guard<std::mutex> lk(dev->mu);  // the corpora's device state is read under the lock
  if (!dst->d || dst->d->ordinal != dev->ordinal) return fail(KPE_E_STATE, "kpe_results_gather: dst is not uploaded to this device");
  for (int t = 0; t < nsrcs; ++t)
    if (!srcs[t]->d || srcs[t]->d->ordinal != dev->ordinal)
      return fail(KPE_E_STATE, "kpe_results_gather: a source is not uploaded to this device");
  // what every listed source keeps; the first listed source's names are the reference
  bool all_m = true, all_f = true;
  const kpe::DeviceCorpus* first = nullptr;
  for (int t = 0; t < nsrcs; ++t) {
    if (!listed[t]) continue;
    const kpe::DeviceCorpus& S = *srcs[t]->d;
    all_m = all_m && S.kept_rules >= 0, all_f = all_f && S.fps_kept;
    if (!first) first = &S;
  }
  if ((what & KPE_GATHER_MATRIX) && !all_m) return fail(KPE_E_STATE, "kpe_results_gather: a listed source keeps no matrix");
  if ((what & KPE_GATHER_FINGERPRINTS) && !all_f)
    return fail(KPE_E_STATE, "kpe_results_gather: a listed source keeps no fingerprints");
  if (!what) what = (all_m ? KPE_GATHER_MATRIX : 0u) | (all_f ? KPE_GATHER_FINGERPRINTS : 0u);
  if (what & KPE_GATHER_MATRIX)
    for (int t = 0; t < nsrcs; ++t)
      if (listed[t] && (srcs[t]->d->kept_rules != first->kept_rules || srcs[t]->d->kept_names != first->kept_names))
        return fail(KPE_E_STATE, "kpe_results_gather: the listed sources' kept rule names differ");
  if (!what) return KPE_OK;
  HIPCHK(hipSetDevice(dev->ordinal));
  kpe::DeviceCorpus& D = *dst->d;
  // behind every listed source's pending keep (enqueued on the stream of its last evaluation)
  for (int t = 0; t < nsrcs; ++t)
    if (listed[t]) HIPCHK(hipStreamSynchronize(srcs[t]->d->bind.last ? srcs[t]->d->bind.last : dev->stream));
  hipStream_t s = D.bind.last ? D.bind.last : dev->stream;
  // this call's scratch: the pair list, then one base pointer per source and kind
  const size_t pair_bytes = (size_t)npairs * 16, tab_bytes = (size_t)nsrcs * 8;
  DevBuf scratch;
  HIPCHK(scratch.ensure(pair_bytes + 2 * tab_bytes));
  uint64_t* d_pairs = scratch.as<uint64_t>();
  std::vector<const void*> tab(2 * (size_t)nsrcs, nullptr);
  for (int t = 0; t < nsrcs; ++t) {
    if (!listed[t]) continue;
    if (what & KPE_GATHER_MATRIX) tab[t] = srcs[t]->d->kept.p;
    if (what & KPE_GATHER_FINGERPRINTS) tab[(size_t)nsrcs + t] = srcs[t]->d->fps.p;
  }
  if (npairs) HIPCHK(hipMemcpyAsync(d_pairs, pairs, pair_bytes, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(scratch.as<uint8_t>() + pair_bytes, tab.data(), 2 * tab_bytes, hipMemcpyHostToDevice, s));
  const uint8_t* const* d_tab_m = reinterpret_cast<const uint8_t* const*>(scratch.as<uint8_t>() + pair_bytes);
  const uint64_t* const* d_tab_f = reinterpret_cast<const uint64_t* const*>(scratch.as<uint8_t>() + pair_bytes + tab_bytes);
  if (what & KPE_GATHER_MATRIX) {
    const size_t R = (size_t)first->kept_rules;
    D.kept_rules = -1;
    D.splice_valid = false;
    HIPCHK(D.kept.ensure((size_t)npairs * R));
    HIPCHK(kpe_launch_results_gather(d_tab_m, d_pairs, npairs, (uint32_t)R, D.kept.as<uint8_t>(), s));
    D.kept_names = first->kept_names;
    D.kept_rules = (int64_t)R;
  }
  if (what & KPE_GATHER_FINGERPRINTS) {
    D.fps_kept = false;
    HIPCHK(D.fps.ensure((size_t)npairs * 8));
    HIPCHK(kpe_launch_fp_gather_pairs(d_tab_f, d_pairs, npairs, D.fps.as<uint64_t>(), s));
    D.fps_tbl.clear();
    D.fps_kept = true;
  }
  HIPCHK(hipStreamSynchronize(s));  // the scratch and the caller's pairs are this call's
  return KPE_OK;
}

static kpe_status changed_fp_impl(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, const uint64_t* salts,
                                  const uint64_t* msg_salts, uint8_t msg_codes, uint32_t flags, uint64_t* rows_out,
                                  uint8_t* vrows_out, uint64_t* fps_out, uint64_t cap, uint64_t* total_out) {
  *total_out = 0;
  if (!dev || !prog || !c) return fail(KPE_E_INVALID, "null argument");
  if (cap && !rows_out) return fail(KPE_E_INVALID, "cap > 0 without a rows buffer");
  std::vector<uint64_t> tbl;
  if (kpe_status st = fp_table(prog, salts, msg_salts, flags, tbl)) return st;
  if (!c->d || !c->d->fps_kept) return fail(KPE_E_STATE, "no kept fingerprints on this corpus");
  const size_t R = tbl.size() / 2;
  const uint64_t n = (uint64_t)c->c->n;
  std::lock_guard<std::mutex> lk(dev->mu);
  if (kpe_status st = fp_bound(dev, prog, c, flags)) return st;
  if (!n) return KPE_OK;
  kpe::DeviceCorpus& D = *c->d;
  auto& B = D.bind;
  hipStream_t s = B.last ? B.last : dev->stream;
  // the device's scratch: the new fingerprints, the row flags as an N x 1 matrix for the selection
  // chain, its tile offsets and counts, its one mask, the table
  const uint64_t ntiles = (n + 4095u) / 4096u;
  const size_t fp_bytes = (size_t)((n + 1u) & ~(uint64_t)1u) * 8;
  const size_t flag_bytes = (size_t)((n + 15u) & ~(uint64_t)15u);
  const size_t off_bytes = (size_t)((ntiles + 2) & ~(uint64_t)1) * 8;
  const size_t cnt_bytes = (size_t)((ntiles + 3) & ~(uint64_t)3) * 4;
  DevBuf& scratch = dev->fp_scratch;
  DevBuf drows, dverd, dfps;
  HIPCHK(scratch.ensure(fp_bytes + flag_bytes + off_bytes + cnt_bytes + 16 + R * 16));
  uint8_t* base = scratch.as<uint8_t>();
  uint64_t* d_new = reinterpret_cast<uint64_t*>(base);
  uint8_t* d_flags = base + fp_bytes;
  uint64_t* d_off = reinterpret_cast<uint64_t*>(base + fp_bytes + flag_bytes);
  uint32_t* d_cnt = reinterpret_cast<uint32_t*>(base + fp_bytes + flag_bytes + off_bytes);
  uint8_t* d_sel = base + fp_bytes + flag_bytes + off_bytes + cnt_bytes;
  uint64_t* d_tbl = reinterpret_cast<uint64_t*>(d_sel + 16);
  const uint8_t sel1 = (uint8_t)KPE_SEL(1);
  HIPCHK(hipMemcpyAsync(d_sel, &sel1, 1, hipMemcpyHostToDevice, s));
  if (kpe_status st = fp_compute(dev, prog, c, tbl.data(), msg_codes, flags, 0, n, d_tbl, d_new, s)) {
    (void)hipStreamSynchronize(s);
    return st;
  }
  HIPCHK(kpe_launch_fp_diff(d_new, D.fps.as<uint64_t>(), n, d_flags, s));
  HIPCHK(kpe_launch_select_count(d_flags, n, 1u, d_sel, 0, d_cnt, d_off, s));
  uint64_t total = 0;
  HIPCHK(hipMemcpyAsync(&total, d_off + ntiles, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *total_out = total;
  const uint64_t m = std::min(total, cap);
  if (!m) return KPE_OK;
  HIPCHK(drows.ensure((size_t)m * 8));
  HIPCHK(kpe_launch_select_scatter(d_flags, n, 1u, d_sel, 0, d_off, m, drows.as<uint64_t>(), nullptr, s));
  const bool vr = vrows_out && R;
  if (vr) {
    HIPCHK(dverd.ensure((size_t)m * R));
    HIPCHK(kpe_launch_gather_rows(B.verdicts.as<uint8_t>(), (uint32_t)R, drows.as<uint64_t>(), m, dverd.as<uint8_t>(), s));
  }
  if (fps_out) {
    HIPCHK(dfps.ensure((size_t)m * 8));
    HIPCHK(kpe_launch_fp_gather(d_new, drows.as<uint64_t>(), m, dfps.as<uint64_t>(), s));
  }
  HIPCHK(hipMemcpyAsync(rows_out, drows.p, (size_t)m * 8, hipMemcpyDeviceToHost, s));
  if (vr) HIPCHK(hipMemcpyAsync(vrows_out, dverd.p, (size_t)m * R, hipMemcpyDeviceToHost, s));
  if (fps_out) HIPCHK(hipMemcpyAsync(fps_out, dfps.p, (size_t)m * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return KPE_OK;
}

int64_t kpe_changed_rows_fp(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, const uint64_t* salts,
                            const uint64_t* msg_salts, uint8_t msg_codes, uint32_t flags, uint64_t* rows,
                            uint8_t* verdict_rows, uint64_t* fps_out, uint64_t cap) {
  uint64_t total = 0;
  const kpe_status st =
      changed_fp_impl(dev, prog, c, salts, msg_salts, msg_codes, flags, rows, verdict_rows, fps_out, cap, &total);
  return st ? -(int64_t)st : (int64_t)total;
}

static kpe_status changed_pairs_fp_impl(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c_new,
                                        const kpe_corpus* c_old, const uint64_t* pairs, uint64_t npairs,
                                        const uint64_t* salts, const uint64_t* msg_salts, uint8_t msg_codes, uint32_t flags,
                                        uint64_t* changed_out, uint8_t* vrows_out, uint64_t* fps_out, uint64_t cap,
                                        uint64_t* total_out) {
  *total_out = 0;
  if (kpe_status st = pairs_args(dev, prog, c_new, c_old, pairs, npairs, changed_out, cap)) return st;
  std::vector<uint64_t> tbl;
  if (kpe_status st = fp_table(prog, salts, msg_salts, flags, tbl)) return st;
  if (!c_old->d || !c_old->d->fps_kept) return fail(KPE_E_STATE, "no kept fingerprints on this corpus");
  const size_t R = tbl.size() / 2;
  std::lock_guard<std::mutex> lk(dev->mu);
  if (!c_new->d) return fail(KPE_E_STATE, "corpus not uploaded");
  if (kpe_status st = fp_bound(dev, prog, c_new, flags)) return st;
  hipStream_t s = nullptr;
  if (kpe_status st = pairs_bound(dev, prog, c_new, c_old, &s)) return st;
  if (!npairs) return KPE_OK;
  auto& B = c_new->d->bind;
  const size_t fp_bytes = (size_t)((npairs + 1u) & ~(uint64_t)1u) * 8;
  DevBuf scratch, didx, drows, dverd, dfps;  // this call's, freed on every return path
  PairScratch S;
  if (kpe_status st = pairs_scratch(scratch, pairs, npairs, fp_bytes + R * 16, s, &S)) return st;
  uint64_t* d_new = reinterpret_cast<uint64_t*>(S.d_extra);
  uint64_t* d_tbl = d_new + fp_bytes / 8;
  if (R) HIPCHK(hipMemcpyAsync(d_tbl, tbl.data(), R * 16, hipMemcpyHostToDevice, s));
  HIPCHK(kpe_launch_fp_pairs(B.verdicts.as<uint8_t>(), (flags & KPE_FP_MASKS) ? B.masks.as<uint32_t>() : nullptr,
                             (uint32_t)R, S.d_pairs, npairs, d_tbl, msg_codes, c_old->d->fps.as<uint64_t>(), d_new,
                             S.d_flags, s));
  HIPCHK(kpe_launch_select_count(S.d_flags, npairs, 1u, S.d_sel, 0, S.d_cnt, S.d_off, s));
  uint64_t total = 0;
  HIPCHK(hipMemcpyAsync(&total, S.d_off + S.ntiles, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));  // also: pairs and the table are copied
  *total_out = total;
  const uint64_t m = std::min(total, cap);
  if (!m) return KPE_OK;
  HIPCHK(didx.ensure((size_t)m * 8));
  HIPCHK(kpe_launch_select_scatter(S.d_flags, npairs, 1u, S.d_sel, 0, S.d_off, m, didx.as<uint64_t>(), nullptr, s));
  const bool vr = vrows_out && R;
  if (vr) {
    HIPCHK(drows.ensure((size_t)m * 8));
    HIPCHK(dverd.ensure((size_t)m * R));
    HIPCHK(kpe_launch_pair_rows(S.d_pairs, didx.as<uint64_t>(), m, drows.as<uint64_t>(), s));
    HIPCHK(kpe_launch_gather_rows(B.verdicts.as<uint8_t>(), (uint32_t)R, drows.as<uint64_t>(), m, dverd.as<uint8_t>(), s));
  }
  if (fps_out) {
    HIPCHK(dfps.ensure((size_t)m * 8));
    HIPCHK(kpe_launch_fp_gather(d_new, didx.as<uint64_t>(), m, dfps.as<uint64_t>(), s));
  }
  HIPCHK(hipMemcpyAsync(changed_out, didx.p, (size_t)m * 8, hipMemcpyDeviceToHost, s));
  if (vr) HIPCHK(hipMemcpyAsync(vrows_out, dverd.p, (size_t)m * R, hipMemcpyDeviceToHost, s));
  if (fps_out) HIPCHK(hipMemcpyAsync(fps_out, dfps.p, (size_t)m * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return KPE_OK;
}

int64_t kpe_changed_pairs_fp(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c_new, const kpe_corpus* c_old,
                             const uint64_t* pairs, uint64_t npairs, const uint64_t* salts, const uint64_t* msg_salts,
                             uint8_t msg_codes, uint32_t flags, uint64_t* changed, uint8_t* verdict_rows,
                             uint64_t* fps_out, uint64_t cap) {
  uint64_t total = 0;
  const kpe_status st = changed_pairs_fp_impl(dev, prog, c_new, c_old, pairs, npairs, salts, msg_salts, msg_codes, flags,
                                              changed, verdict_rows, fps_out, cap, &total);
  return st ? -(int64_t)st : (int64_t)total;
}

// ---- namespace groups and per-namespace rule counts -------------------------------------------
// the group of row i: its r_nsa id; a row without a namespace string belongs to ""
static inline uint32_t ns_group_of(const kpe::Corpus& C, const NsGroups& G, size_t i) {
  const uint32_t id = i < C.r_nsa.size() ? C.r_nsa[i] : KPE_NO_STR;
  return id < C.dict[D_NS].size() ? id : G.empty;
}

int64_t kpe_corpus_num_namespaces(const kpe_corpus* c) { return c ? (int64_t)ns_groups(c).names.size() : 0; }
const char* kpe_corpus_namespace(const kpe_corpus* c, int64_t g) {
  if (!c) return nullptr;
  const NsGroups& G = ns_groups(c);
  return g >= 0 && (size_t)g < G.names.size() ? G.names[(size_t)g].c_str() : nullptr;
}
kpe_status kpe_corpus_row_namespaces(const kpe_corpus* c, uint32_t* out) {
  if (!c || (!out && c->c->n)) return fail(KPE_E_INVALID, "kpe_corpus_row_namespaces: null argument");
  const NsGroups& G = ns_groups(c);
  for (int64_t i = 0; i < c->c->n; ++i) out[i] = ns_group_of(*c->c, G, (size_t)i);
  return KPE_OK;
}
kpe_status kpe_corpus_namespace_rows(const kpe_corpus* c, uint64_t* out) {
  if (!c || !out) return fail(KPE_E_INVALID, "kpe_corpus_namespace_rows: null argument");
  const NsGroups& G = ns_groups(c);
  std::fill(out, out + G.names.size(), (uint64_t)0);
  for (int64_t i = 0; i < c->c->n; ++i) ++out[ns_group_of(*c->c, G, (size_t)i)];
  return KPE_OK;
}

static inline void ns_count_add(kpe_ns_counts& o, uint8_t v) {
  switch (v) {
    case KPE_PASS: ++o.pass; break;
    case KPE_FAIL: ++o.fail; break;
    case KPE_WARN: ++o.warn; break;
    case KPE_ERROR: ++o.error; break;
    case KPE_SKIP: ++o.skip; break;
    case KPE_UNDECIDED: ++o.undecided; break;
    default: break;  // KPE_NA: no RuleResponse
  }
}

// the argument checks the device call and its host twin share (before any device call)
static kpe_status ns_window_check(const kpe_program* prog, const kpe_corpus* c, uint64_t g0, uint64_t ng,
                                  const void* out) {
  if (!prog || !c || (ng && !out)) return fail(KPE_E_INVALID, "null argument");
  const uint64_t G = ns_groups(c).names.size();
  if (g0 > G || ng > G - g0) return fail(KPE_E_INVALID, "namespace groups past the corpus");
  if ((uint64_t)c->c->n >= (1ull << 32)) return fail(KPE_E_LIMIT, "namespace counts hold at most 2^32 - 1 rows");
  return KPE_OK;
}

kpe_status kpe_namespace_counts_host(const kpe_program* prog, const kpe_corpus* c, const uint8_t* verdicts,
                                     uint64_t g0, uint64_t ng, kpe_ns_counts* out) {
  if (kpe_status st = ns_window_check(prog, c, g0, ng, out)) return st;
  const size_t R = prog->p->rules.size();
  if (!ng || !R) return KPE_OK;
  const kpe::Corpus& C = *c->c;
  if (!verdicts && C.n) return fail(KPE_E_INVALID, "null argument");
  const NsGroups& G = ns_groups(c);
  memset(out, 0, (size_t)ng * R * sizeof(kpe_ns_counts));
  for (int64_t i = 0; i < C.n; ++i) {
    const uint64_t g = ns_group_of(C, G, (size_t)i);
    if (g < g0 || g - g0 >= ng) continue;
    kpe_ns_counts* o = out + (size_t)(g - g0) * R;
    const uint8_t* v = verdicts + (size_t)i * R;
    for (size_t r = 0; r < R; ++r) ns_count_add(o[r], v[r]);
  }
  return KPE_OK;
}

// The corpus's rows-by-namespace index, once per upload: a counting sort of the row ids by group
// (4 bytes per row) and each group's rows cut into work items of at most kpe_ns_chunk_rows() rows.
static kpe_status ns_index(kpe_device* dev, const kpe_corpus* c, hipStream_t s) {
  kpe::DeviceCorpus& D = *c->d;
  if (D.ns_ready) return KPE_OK;
  const auto t0 = std::chrono::steady_clock::now();
  const kpe::Corpus& C = *c->c;
  const NsGroups& G = ns_groups(c);
  const size_t ngr = G.names.size(), n = (size_t)C.n;
  const uint32_t chunk = kpe_ns_chunk_rows();
  std::vector<uint32_t> off(ngr + 1, 0u), rows(n);
  for (size_t i = 0; i < n; ++i) ++off[ns_group_of(C, G, i) + 1u];
  for (size_t g = 0; g < ngr; ++g) off[g + 1] += off[g];
  {
    std::vector<uint32_t> cur(off.begin(), off.end() - 1);
    for (size_t i = 0; i < n; ++i) rows[cur[ns_group_of(C, G, i)]++] = (uint32_t)i;  // ascending rows per group
  }
  std::vector<KpeNsItem> items;
  D.ns_item_off.assign(ngr + 1, 0);
  for (size_t g = 0; g < ngr; ++g) {
    D.ns_item_off[g] = items.size();
    const bool single = off[g + 1] - off[g] <= chunk;
    for (uint32_t b = off[g]; b < off[g + 1]; b += chunk)
      items.push_back(KpeNsItem{(uint32_t)g, b, std::min(b + chunk, off[g + 1]), single ? 1u : 0u});
  }
  D.ns_item_off[ngr] = items.size();
  HIPCHK(D.ns_rows.ensure(rows.size() * 4));
  HIPCHK(D.ns_items.ensure(items.size() * sizeof(KpeNsItem)));
  if (!rows.empty()) HIPCHK(hipMemcpyAsync(D.ns_rows.p, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, s));
  if (!items.empty())
    HIPCHK(hipMemcpyAsync(D.ns_items.p, items.data(), items.size() * sizeof(KpeNsItem), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));  // rows / items are this call's
  D.ns_ready = true;
  dev->ns_index_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return KPE_OK;
}

kpe_status kpe_fetch_namespace_counts(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, uint64_t g0,
                                      uint64_t ng, kpe_ns_counts* out) {
  if (!dev) return fail(KPE_E_INVALID, "null argument");
  if (kpe_status st = ns_window_check(prog, c, g0, ng, out)) return st;
  const size_t R = prog->p->rules.size();
  if (!ng || !R) return KPE_OK;
  if (!c->d) return fail(KPE_E_STATE, "corpus not uploaded");
  std::lock_guard<std::mutex> lk(dev->mu);
  HIPCHK(hipSetDevice(dev->ordinal));
  auto& B = c->d->bind;
  if (B.prog != prog->p.get()) return fail(KPE_E_STATE, "no evaluation of this program on this corpus");
  if (c->d->ordinal != dev->ordinal) return fail(KPE_E_STATE, "corpus not uploaded to this device");
  hipStream_t s = B.last ? B.last : dev->stream;
  if (kpe_status st = ns_index(dev, c, s)) return st;
  kpe::DeviceCorpus& D = *c->d;
  static_assert(sizeof(kpe_ns_counts) == 24, "6 words per (group, rule)");
  const size_t out_bytes = (size_t)ng * R * sizeof(kpe_ns_counts);
  // the window's counters: a table of up to kNsKeepBytes stays with the corpus (a consumer asks
  // for the same small table after every evaluation: no allocation per call); a larger window is
  // this call's scratch, freed on every return path
  constexpr size_t kNsKeepBytes = 4u << 20;
  DevBuf own;
  DevBuf& scratch = out_bytes <= kNsKeepBytes ? D.ns_out : own;
  HIPCHK(scratch.ensure(out_bytes));
  HIPCHK(hipMemsetAsync(scratch.p, 0, out_bytes, s));
  const uint64_t i0 = D.ns_item_off[g0], i1 = D.ns_item_off[g0 + ng];  // the window's work items
  hipEvent_t ea = nullptr, eb = nullptr;
  if (dev->timing) {
    ea = dev->get_ev(), eb = dev->get_ev();
    HIPCHK(hipEventRecord(ea, s));
  }
  HIPCHK(kpe_launch_ns_counts(B.verdicts.as<uint8_t>(), (uint32_t)R, D.ns_rows.as<uint32_t>(),
                              D.ns_items.as<KpeNsItem>() + i0, i1 - i0, (uint32_t)g0, scratch.as<uint32_t>(), s));
  if (dev->timing) HIPCHK(hipEventRecord(eb, s));
  HIPCHK(hipMemcpyAsync(out, scratch.p, out_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (dev->timing) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ea, eb) == hipSuccess) dev->ns_kernel_ms = ms;
    dev->pool.push_back(ea), dev->pool.push_back(eb);
  }
  return KPE_OK;
}
// Diagnostic (not in kpe.h; scripts/ns_counts_bench.py): with kpe_device_set_timing on, the kernel
// time of the last kpe_fetch_namespace_counts and the last index build + upload, in ms
kpe_status kpe_debug_ns_counts_ms(kpe_device* dev, double* kernel_ms, double* index_ms) {
  if (!dev) return fail(KPE_E_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(dev->mu);
  if (kernel_ms) *kernel_ms = dev->ns_kernel_ms;
  if (index_ms) *index_ms = dev->ns_index_ms;
  return KPE_OK;
}

// ---- failing paths of pattern cells (report time) ---------------------------------------------
// The condition trace slot of every rule (kernels_abi.h KPE_RR_SLOT): where its words start in a
// row's nmsg words and how many it has (kpe_fetch_cond_traces_ex's expansion, per rule)
static std::vector<uint32_t> cond_slot_table(const kpe::Program& P) {
  std::vector<uint32_t> slot(P.rules.size(), 0u);
  for (const KpeCRule& cr : P.cond.rules)
    if (cr.mslot) slot[cr.col] = KPE_RR_SLOT(cr.mslot - 1u, cr.kind == CR_FOREACH ? KPE_FE_TRACE_WORDS : 1u);
  return slot;
}
// The pattern trace jobs of listed cells (kpe_launch_pattern_trace): w holds KPE_FE_TRACE_WORDS
// condition trace words per cell, cells[i] % R is the cell's rule. A FAIL / ERROR cell of a validate.foreach
// rule that a pattern entry decided walks that entry's roots on the element it validated; every
// other cell's job stays zero. jobs is left empty when no cell has one.
static void fe_pat_jobs(const kpe::Program& P, const std::vector<uint32_t>& slot, const uint64_t* cells, const uint32_t* w,
                        uint64_t ncells, std::vector<uint4>& jobs) {
  const size_t R = P.rules.size();
  for (uint64_t i = 0; i < ncells; ++i, w += KPE_FE_TRACE_WORDS) {
    const uint32_t c = (uint32_t)(cells[i] % R);
    if (KPE_RR_SLOT_WIDTH(slot[c]) != KPE_FE_TRACE_WORDS) continue;
    if (jobs.empty()) jobs.assign(ncells, make_uint4(0u, 0u, 0u, 0u));
    if (FT_KIND(w[1]) != FT_PAT || w[3] == 0xFFFFFFFEu) continue;
    const int64_t e = fe_decider(P, P.reports[c], w[1]);
    if (e < 0) continue;
    const KpeCForeach& fe = P.cond.fes[(size_t)e];
    if (fe.kind != FE_PAT) continue;
    jobs[i] = make_uint4(fe.a, fe.b, w[3], 1u);
  }
}

kpe_status kpe_pattern_traces(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, const uint64_t* cells,
                              uint64_t ncells, uint32_t* out) {
  if (!dev || !prog || !c || !c->d || (ncells && (!cells || !out))) return fail(KPE_E_INVALID, "null argument");
  if (!ncells) return KPE_OK;
  std::lock_guard<std::mutex> lk(dev->mu);
  HIPCHK(hipSetDevice(dev->ordinal));
  auto& B = c->d->bind;
  const kpe::Program& P = *prog->p;
  if (B.prog != prog->p.get()) return fail(KPE_E_STATE, "no evaluation of this program on this corpus");
  if (c->d->ordinal != dev->ordinal) return fail(KPE_E_STATE, "corpus not uploaded to this device");
  const size_t R = P.rules.size();
  const uint64_t total = (uint64_t)c->c->n * R;
  for (uint64_t i = 0; i < ncells; ++i)
    if (cells[i] >= total) return fail(KPE_E_INVALID, "cell index past the verdict matrix");
  const size_t rec = (size_t)KPE_TRACE_ROOTS * KPE_TRACE_WORDS;
  hipStream_t s = B.last ? B.last : dev->stream;
  // foreach cells decided by a pattern entry: the entry's roots on the element (the condition
  // kernel's trace words of the cells: one gather, one copy)
  std::vector<uint4> jobs;
  if (P.any_fe_pat && B.cargs_valid && P.cond.nmsg) {
    const std::vector<uint32_t> slot = cond_slot_table(P);
    DevBuf dcl, dsl, dw;
    std::vector<uint32_t> w(ncells * KPE_FE_TRACE_WORDS);
    HIPCHK(dcl.ensure(ncells * 8));
    HIPCHK(dsl.ensure(R * 4));
    HIPCHK(dw.ensure(w.size() * 4));
    HIPCHK(hipMemcpyAsync(dcl.p, cells, ncells * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dsl.p, slot.data(), R * 4, hipMemcpyHostToDevice, s));
    HIPCHK(kpe_launch_fe_words_gather(dcl.as<uint64_t>(), ncells, (uint32_t)R, dsl.as<uint32_t>(),
                                      B.mtrace.as<uint32_t>(), P.cond.nmsg, dw.as<uint32_t>(), s));
    HIPCHK(hipMemcpyAsync(w.data(), dw.p, w.size() * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    fe_pat_jobs(P, slot, cells, w.data(), ncells, jobs);
  }
  if (P.pat.rules.empty() && jobs.empty()) {  // no pattern walk: every record is empty
    memset(out, 0, ncells * rec * 4);
    return KPE_OK;
  }
  if (!B.pargs_valid) return fail(KPE_E_STATE, "the binding has no completed evaluation of its pattern rules");
  void *dc = nullptr, *dout = nullptr, *dj = nullptr;
  hipError_t e = hipMalloc(&dc, ncells * 8);
  if (e == hipSuccess) e = hipMalloc(&dout, ncells * rec * 4);
  if (e == hipSuccess && !jobs.empty()) e = hipMalloc(&dj, ncells * sizeof(uint4));
  if (e == hipSuccess) e = hipMemcpyAsync(dc, cells, ncells * 8, hipMemcpyHostToDevice, s);
  if (e == hipSuccess && dj) e = hipMemcpyAsync(dj, jobs.data(), ncells * sizeof(uint4), hipMemcpyHostToDevice, s);
  if (e == hipSuccess)
    e = kpe_launch_pattern_trace(B.pargs.as<PatArgs>(), (const uint64_t*)dc, ncells, (uint32_t*)dout,
                                 (const uint4*)dj, s);
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout, ncells * rec * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (dc) (void)hipFree(dc);
  if (dout) (void)hipFree(dout);
  if (dj) (void)hipFree(dj);
  HIPCHK(e);
  return KPE_OK;
}

// ---- condition traces (report time) -----------------------------------------------------------
kpe_status kpe_fetch_cond_traces(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, uint64_t row0,
                                 uint64_t nrows, uint32_t* out) {
  if (!dev || !prog || !c || !c->d || (nrows && !out)) return fail(KPE_E_INVALID, "null argument");
  if (row0 > (uint64_t)c->c->n || nrows > (uint64_t)c->c->n - row0) return fail(KPE_E_INVALID, "rows past the corpus");
  if (!nrows) return KPE_OK;
  const kpe::Program& P = *prog->p;
  const size_t R = P.rules.size();
  memset(out, 0, nrows * R * 4);
  if (!P.cond.nmsg) return KPE_OK;
  std::lock_guard<std::mutex> lk(dev->mu);
  HIPCHK(hipSetDevice(dev->ordinal));
  auto& B = c->d->bind;
  if (B.prog != prog->p.get() || !B.cargs_valid)
    return fail(KPE_E_STATE, "no evaluation of this program on this corpus");
  if (c->d->ordinal != dev->ordinal) return fail(KPE_E_STATE, "corpus not uploaded to this device");
  const size_t m = P.cond.nmsg;
  std::vector<uint32_t> h(nrows * m);
  hipStream_t s = B.last ? B.last : dev->stream;
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipMemcpy(h.data(), B.mtrace.as<uint32_t>() + row0 * m, h.size() * 4, hipMemcpyDeviceToHost));
  for (const KpeCRule& cr : P.cond.rules)
    if (cr.mslot)
      for (uint64_t i = 0; i < nrows; ++i) out[i * R + cr.col] = h[i * m + cr.mslot - 1u];
  return KPE_OK;
}

kpe_status kpe_fetch_cond_traces_ex(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, uint64_t row0,
                                    uint64_t nrows, uint32_t* out) {
  if (!dev || !prog || !c || !c->d || (nrows && !out)) return fail(KPE_E_INVALID, "null argument");
  if (row0 > (uint64_t)c->c->n || nrows > (uint64_t)c->c->n - row0) return fail(KPE_E_INVALID, "rows past the corpus");
  if (!nrows) return KPE_OK;
  const kpe::Program& P = *prog->p;
  const size_t R = P.rules.size(), W = KPE_CTRACE_WORDS;
  memset(out, 0, nrows * R * W * 4);
  if (!P.cond.nmsg) return KPE_OK;
  std::lock_guard<std::mutex> lk(dev->mu);
  HIPCHK(hipSetDevice(dev->ordinal));
  auto& B = c->d->bind;
  if (B.prog != prog->p.get() || !B.cargs_valid)
    return fail(KPE_E_STATE, "no evaluation of this program on this corpus");
  if (c->d->ordinal != dev->ordinal) return fail(KPE_E_STATE, "corpus not uploaded to this device");
  const size_t m = P.cond.nmsg;
  std::vector<uint32_t> h(nrows * m);
  hipStream_t s = B.last ? B.last : dev->stream;
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipMemcpy(h.data(), B.mtrace.as<uint32_t>() + row0 * m, h.size() * 4, hipMemcpyDeviceToHost));
  for (const KpeCRule& cr : P.cond.rules) {
    if (!cr.mslot) continue;
    const size_t nw = cr.kind == CR_FOREACH ? KPE_FE_TRACE_WORDS : 1u;
    for (uint64_t i = 0; i < nrows; ++i)
      for (size_t w = 0; w < nw; ++w) out[(i * R + cr.col) * W + w] = h[i * m + cr.mslot - 1u + w];
  }
  return KPE_OK;
}

// ---- report detail of a row list: the sparse fetch (need tables and rendering: report.cpp) ------
kpe_status kpe_fetch_report_rows(kpe_device* dev, const kpe_program* prog, const kpe_corpus* c, const uint64_t* rows,
                                 uint64_t nrows, uint32_t flags, kpe_report_rows* io) {
  if (!dev || !prog || !c || (nrows && !rows)) return fail(KPE_E_INVALID, "null argument");
  kpe_status st = report_rows_args(flags, io, true);
  if (st) return st;
  io->mask_total = io->cond_total = io->pattern_total = 0;
  const kpe::Program& P = *prog->p;
  const size_t R = P.rules.size();
  const uint64_t N = (uint64_t)c->c->n;
  for (uint64_t k = 0; k < nrows; ++k)
    if (rows[k] >= N) return fail(KPE_E_INVALID, "row past the corpus");
  const uint64_t cells = nrows * R;
  if (!cells) return KPE_OK;
  if (!c->d) return fail(KPE_E_STATE, "corpus not uploaded");
  std::vector<uint8_t> need;
  if ((st = report_need_tables(prog, flags, need))) return st;
  std::lock_guard<std::mutex> lk(dev->mu);
  HIPCHK(hipSetDevice(dev->ordinal));
  auto& B = c->d->bind;
  if (B.prog != prog->p.get()) return fail(KPE_E_STATE, "no evaluation of this program on this corpus");
  if (c->d->ordinal != dev->ordinal) return fail(KPE_E_STATE, "corpus not uploaded to this device");
  if ((flags & KPE_RR_MASKS) && !c->d->has_masks) return fail(KPE_E_STATE, "check masks were not computed");
  const uint32_t nmsg = P.cond.nmsg;
  if ((flags & KPE_RR_COND) && nmsg && !B.cargs_valid)
    return fail(KPE_E_STATE, "no evaluation of this program on this corpus");
  const std::vector<uint32_t> slot = cond_slot_table(P);
  for (size_t r = 0; r < R; ++r)  // a slot lies inside the row's words, or the rule has none
    if (KPE_RR_SLOT_WIDTH(slot[r]) && KPE_RR_SLOT_FIRST(slot[r]) + KPE_RR_SLOT_WIDTH(slot[r]) > nmsg)
      return fail(KPE_E_INVALID, "condition trace slot past the row's words");
    else if (!KPE_RR_SLOT_WIDTH(slot[r])) need[R + r] = 0;
  hipStream_t s = B.last ? B.last : dev->stream;

  // stage 1 (rr_scratch): the row list, the compact matrix, the tiles, the tables
  auto a16 = [](size_t x) { return (x + 15u) & ~(size_t)15u; };
  const uint64_t ntiles = kpe_report_need_tiles(cells);
  const size_t o_rows = 0, o_v = o_rows + a16(nrows * 8), o_cnt = o_v + a16(cells);
  const size_t o_off = o_cnt + a16((3 * ntiles + 3) / 4 * 16), o_need = o_off + a16((3 * ntiles + 1) * 8);
  const size_t o_slot = o_need + a16(3 * R), s1_bytes = o_slot + a16(4 * R);
  HIPCHK(dev->rr_scratch.ensure(s1_bytes));
  uint8_t* s1 = dev->rr_scratch.as<uint8_t>();
  uint64_t* d_rows = reinterpret_cast<uint64_t*>(s1 + o_rows);
  uint8_t* d_v = s1 + o_v;
  uint32_t* d_cnt = reinterpret_cast<uint32_t*>(s1 + o_cnt);
  uint64_t* d_off = reinterpret_cast<uint64_t*>(s1 + o_off);
  uint8_t* d_need = s1 + o_need;
  uint32_t* d_slot = reinterpret_cast<uint32_t*>(s1 + o_slot);
  HIPCHK(hipMemcpyAsync(d_rows, rows, nrows * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d_need, need.data(), 3 * R, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d_slot, slot.data(), 4 * R, hipMemcpyHostToDevice, s));
  HIPCHK(kpe_launch_gather_rows(B.verdicts.as<uint8_t>(), (uint32_t)R, d_rows, nrows, d_v, s));
  HIPCHK(kpe_launch_report_need_count(d_v, cells, (uint32_t)R, d_need, d_cnt, d_off, s));
  uint64_t ends[4] = {0, 0, 0, 0};  // offs[0], offs[ntiles], offs[2 ntiles], offs[3 ntiles]: one strided copy
  HIPCHK(hipMemcpy2DAsync(ends, 8, d_off, (size_t)ntiles * 8, 8, 4, hipMemcpyDeviceToHost, s));
  if (io->verdict_rows) HIPCHK(hipMemcpyAsync(io->verdict_rows, d_v, cells, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  io->mask_total = ends[1] - ends[0], io->cond_total = ends[2] - ends[1], io->pattern_total = ends[3] - ends[2];
  const uint64_t mm = (flags & KPE_RR_MASKS) ? std::min(io->mask_total, io->mask_cap) : 0;
  const uint64_t mc = (flags & KPE_RR_COND) ? std::min(io->cond_total, io->cond_cap) : 0;
  const uint64_t mp = (flags & KPE_RR_PATTERNS) ? std::min(io->pattern_total, io->pattern_cap) : 0;
  if (!(mm | mc | mp)) return KPE_OK;

  // stage 2 (rr_out): the lists and their payloads, sized by what is written
  const size_t rec = (size_t)KPE_TRACE_ROOTS * KPE_TRACE_WORDS * 4;
  const size_t o_mcell = 0, o_ccell = o_mcell + a16(mm * 8), o_pcell = o_ccell + a16(mc * 8);
  const size_t o_pabs = o_pcell + a16(mp * 8);
  const size_t o_cw = o_pabs + a16(mp * 8), o_job = o_cw + a16(mc * 16), o_few = o_job + a16(mp * 16);
  const size_t o_rec = o_few + a16(mp * 16), o_mw = o_rec + a16(mp * rec), s2_bytes = o_mw + a16(mm * 4);
  HIPCHK(dev->rr_out.ensure(s2_bytes));
  uint8_t* s2 = dev->rr_out.as<uint8_t>();
  KpeRrSrc src{d_rows, B.masks.as<uint32_t>(), B.mtrace.as<uint32_t>(), d_slot, nmsg, 0u};
  KpeRrOut out{reinterpret_cast<uint64_t*>(s2 + o_mcell), reinterpret_cast<uint32_t*>(s2 + o_mw), mm,
               reinterpret_cast<uint64_t*>(s2 + o_ccell), reinterpret_cast<uint32_t*>(s2 + o_cw), mc,
               reinterpret_cast<uint64_t*>(s2 + o_pcell), reinterpret_cast<uint64_t*>(s2 + o_pabs), mp};
  HIPCHK(kpe_launch_report_need_scatter(d_v, cells, (uint32_t)R, d_need, d_off, &src, &out, s));
  if (mm) {
    HIPCHK(hipMemcpyAsync(io->mask_cells, out.mask_cells, mm * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(io->mask_words, out.mask_words, mm * 4, hipMemcpyDeviceToHost, s));
  }
  if (mc) {
    HIPCHK(hipMemcpyAsync(io->cond_cells, out.cond_cells, mc * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(io->cond_words, out.cond_words, mc * 16, hipMemcpyDeviceToHost, s));
  }
  if (mp) {
    HIPCHK(hipMemcpyAsync(io->pattern_cells, out.pattern_cells, mp * 8, hipMemcpyDeviceToHost, s));
    // foreach cells decided by a pattern entry: their jobs from their trace words, as kpe_pattern_traces
    std::vector<uint4> jobs;
    if (P.any_fe_pat && B.cargs_valid && nmsg) {
      std::vector<uint32_t> w(mp * KPE_FE_TRACE_WORDS);
      uint32_t* d_few = reinterpret_cast<uint32_t*>(s2 + o_few);
      HIPCHK(kpe_launch_fe_words_gather(out.pattern_abs, mp, (uint32_t)R, d_slot, B.mtrace.as<uint32_t>(), nmsg, d_few, s));
      HIPCHK(hipMemcpyAsync(w.data(), d_few, w.size() * 4, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      fe_pat_jobs(P, slot, io->pattern_cells, w.data(), mp, jobs);
    }
    if (P.pat.rules.empty() && jobs.empty()) {  // no pattern walk: every record is empty
      memset(io->pattern_traces, 0, mp * rec);
    } else {
      if (!B.pargs_valid) return fail(KPE_E_STATE, "the binding has no completed evaluation of its pattern rules");
      uint4* d_job = reinterpret_cast<uint4*>(s2 + o_job);
      uint32_t* d_rec = reinterpret_cast<uint32_t*>(s2 + o_rec);
      if (!jobs.empty()) HIPCHK(hipMemcpyAsync(d_job, jobs.data(), mp * sizeof(uint4), hipMemcpyHostToDevice, s));
      HIPCHK(kpe_launch_pattern_trace(B.pargs.as<PatArgs>(), out.pattern_abs, mp, d_rec, jobs.empty() ? nullptr : d_job,
                                      s));
      HIPCHK(hipMemcpyAsync(io->pattern_traces, d_rec, mp * rec, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));  // jobs is read by the upload until here
    }
  }
  HIPCHK(hipStreamSynchronize(s));
  return KPE_OK;
}

}  // extern "C"
