// Host check of kpe_corpus_gather and kpe_results_gather under ASan / UBSan, for
// tests/test_corpus_gather_host.py without a GPU. Not part of libkpe:
//   scripts/build/corpus_gather_check [<ndjson> <ns_labels_json>]
// 1. The kernel body (kyverno_amd/csrc/gather.inl, the text kpe_results_gather_kernel and
//    kpe_fp_gather_pairs_kernel run), the 256 lanes of each block in turn, over source buffers of
//    exactly N x R bytes (N x 8 for the fingerprints) and outputs of exactly npairs x R (npairs x 8)
//    bytes, for R in {1, 3, 4, 5, 17, 204} x npairs in {1, 63, 64, 65, 1000} and three grids, against
//    the plain double loop. A source no pair names has a null base. Every word store is counted: an
//    output byte is written once.
// 2. With the two files: the host gather (flatten.cpp gather_rows) over the NDJSON cut at line
//    boundaries into chunks of 1, 63, 64, 65 rows and the rest, with and without documents. All rows
//    in order: every column, dictionary and table equals the whole flatten's. A shuffled subset
//    (seed 5, about 20 % dropped, one pair twice): row digests, flags, namespaces by name and the
//    label table equal those of a fresh flatten of the same lines, and each row's digest its source's.
// Prints "corpus_gather_check ok" and exits 0, or the first difference and 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../kyverno_amd/csrc/corpus.hpp"
#include "../kyverno_amd/csrc/schema.h"

static int g_bad = 0;
#define CHECK(c, ...)                              \
  do {                                             \
    if (!(c)) {                                    \
      if (!g_bad) {                                \
        fprintf(stderr, "corpus_gather_check: ");  \
        fprintf(stderr, __VA_ARGS__);              \
        fprintf(stderr, "\n");                     \
      }                                            \
      ++g_bad;                                     \
    }                                              \
  } while (0)

// ---- 1. the kernel body ----
static uint8_t* g_out = nullptr;  // the output under test and its per-byte store counts
static std::vector<uint8_t> g_writes;
#define KPE_GA_FN static inline
#define KPE_GA_DEV static inline
static inline uint32_t ga_load4(const uint8_t* p) {
  if (((uintptr_t)p & 3u) != 0) fprintf(stderr, "corpus_gather_check: misaligned word load\n"), exit(2);
  uint32_t w;
  memcpy(&w, p, 4);
  return w;
}
static inline void ga_store4(uint8_t* p, uint32_t w) {
  if (((uintptr_t)p & 3u) != 0) fprintf(stderr, "corpus_gather_check: misaligned word store\n"), exit(2);
  memcpy(p, &w, 4);
  for (int j = 0; j < 4; ++j) ++g_writes[(size_t)(p - g_out) + j];
}
#include "../kyverno_amd/csrc/gather.inl"

template <class T>
static T* exact(size_t n) {  // exactly n elements, aligned like a device allocation
  T* p = static_cast<T*>(malloc(n ? n * sizeof(T) : 1));
  if (!p || ((uintptr_t)p & 15u) != 0) fprintf(stderr, "corpus_gather_check: malloc\n"), exit(2);
  return p;
}

static void kernel_cases() {
  std::mt19937_64 rng(0x6761746865ull);
  const uint64_t srcN[4] = {1, 37, 400, 9};  // source 3 is named by no pair: its base is null
  for (uint32_t R : {1u, 3u, 4u, 5u, 17u, 204u})
    for (uint64_t npairs : {1ull, 63ull, 64ull, 65ull, 1000ull}) {
      uint8_t* src[4] = {};
      uint64_t* fsrc[4] = {};
      for (int t = 0; t < 3; ++t) {
        src[t] = exact<uint8_t>(srcN[t] * R), fsrc[t] = exact<uint64_t>(srcN[t]);
        for (uint64_t i = 0; i < srcN[t] * R; ++i) src[t][i] = (uint8_t)rng();
        for (uint64_t i = 0; i < srcN[t]; ++i) fsrc[t][i] = rng();
      }
      uint64_t* pairs = exact<uint64_t>(2 * npairs);
      for (uint64_t k = 0; k < npairs; ++k) {
        const uint64_t t = k == 0 ? 0 : 1 + rng() % 2;  // source 0's only row first; rows repeat
        pairs[2 * k] = t, pairs[2 * k + 1] = rng() % srcN[t];
      }
      const uint64_t total = npairs * R;
      for (uint32_t grid : {ga_grid(total), 3u, kGaGrid}) {
        uint8_t* out = exact<uint8_t>(total);
        memset(out, 0xEE, total);
        g_out = out, g_writes.assign(total, 0);
        uint64_t covered = 0;
        for (uint32_t b = 0; b < grid; ++b) {
          const GaRange G = ga_range(total, grid, b);
          CHECK(G.b0 == covered && G.b1 >= G.b0 && G.b1 <= total && (G.b0 == total || (G.b0 & 15u) == 0), "R=%u npairs=%llu grid=%u: range %u", R,
                (unsigned long long)npairs, grid, b);
          covered = G.b1;
          for (uint32_t t = 0; t < kGaLanes; ++t) ga_copy(G, t, src, pairs, R, out);
        }
        CHECK(covered == total, "R=%u npairs=%llu grid=%u: the ranges cover %llu of %llu bytes", R, (unsigned long long)npairs,
              grid, (unsigned long long)covered, (unsigned long long)total);
        for (uint64_t k = 0; k < npairs; ++k)
          for (uint32_t c = 0; c < R; ++c) {
            const uint64_t p = k * R + c;
            CHECK(out[p] == src[pairs[2 * k]][pairs[2 * k + 1] * R + c], "R=%u npairs=%llu grid=%u: row %llu column %u", R,
                  (unsigned long long)npairs, grid, (unsigned long long)k, c);
            CHECK(g_writes[p] == (p < (total & ~3ull) ? 1 : 0), "R=%u npairs=%llu grid=%u: byte %llu stored %u times as a word", R,
                  (unsigned long long)npairs, grid, (unsigned long long)p, g_writes[p]);
          }
        free(out);
      }
      uint64_t* fout = exact<uint64_t>(npairs);
      for (uint64_t k = 0; k < npairs; ++k) ga_fp(k, fsrc, pairs, fout);
      for (uint64_t k = 0; k < npairs; ++k)
        CHECK(fout[k] == fsrc[pairs[2 * k]][pairs[2 * k + 1]], "fingerprints, npairs=%llu: row %llu", (unsigned long long)npairs,
              (unsigned long long)k);
      free(fout), free(pairs);
      for (int t = 0; t < 3; ++t) free(src[t]), free(fsrc[t]);
    }
}

// ---- 2. the host gather ----
namespace kpe {
void flatten_ndjson(Corpus& C, const char* buf, size_t len, const char* nsl, size_t nsl_len, bool docs);
void gather_rows(Corpus& C, const std::vector<const Corpus*>& srcs, const uint64_t* pairs, uint64_t npairs);
void row_digests(const Corpus& C, uint64_t* out);
std::string ns_labels_json(const Corpus& C);
}  // namespace kpe
using namespace kpe;

static std::string slurp(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) fprintf(stderr, "corpus_gather_check: cannot read %s\n", path), exit(2);
  std::string s;
  char buf[1 << 16];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) s.append(buf, n);
  fclose(f);
  return s;
}

static bool same_scalars(const Corpus& a, const Corpus& b) {
  return a.scal.size() == b.scal.size() && (a.scal.empty() || !memcmp(a.scal.data(), b.scal.data(), a.scal.size() * sizeof(KpeScalar)));
}

static void same_columns(const Corpus& G, const Corpus& W, const char* what) {
#define SAME(f) CHECK(G.f == W.f, "%s: column " #f " differs from the whole flatten's", what)
  SAME(n); SAME(has_docs);
  for (int d = 0; d < KPE_NUM_DOMAINS; ++d)
    CHECK(G.dict[d].bytes == W.dict[d].bytes && G.dict[d].off == W.dict[d].off, "%s: dictionary %d", what, d);
  SAME(r_flags); SAME(r_gvk); SAME(r_name); SAME(r_mns); SAME(r_nsa); SAME(r_nsl); SAME(limit_rows);
  SAME(lab_off); SAME(lab_k); SAME(lab_v); SAME(ann_off); SAME(ann_k); SAME(ann_v);
  SAME(p_sc); SAME(ctr_off); SAME(vol_off); SAME(vol_src); SAME(sys_off); SAME(sys_id);
  SAME(pann_off); SAME(pann_k); SAME(pann_v); SAME(p_cold);
  SAME(c_sc); SAME(c_add); SAME(c_drop); SAME(c_name); SAME(c_image); SAME(c_sann); SAME(c_sann_key);
  SAME(c_sec_str); SAME(c_pm_str); SAME(c_selt_str); SAME(c_selu_str); SAME(c_selr_str);
  SAME(cport_off); SAME(cport_host); SAME(cport_str);
  SAME(rec); SAME(hdr); SAME(crec); SAME(pann_kv); SAME(capset_add); SAME(capset_drop);
  SAME(nsl_off); SAME(nsl_k); SAME(nsl_v); SAME(nsl_index);
  SAME(doc); SAME(doc_off); SAME(img_off); SAME(scal_text);
#undef SAME
  CHECK(same_scalars(G, W), "%s: the scalar table differs from the whole flatten's", what);
}

static void host_cases(const std::string& nd, const std::string& nsl) {
  std::vector<size_t> line0{0};  // the start of every line, and the end
  for (size_t i = 0; i < nd.size(); ++i)
    if (nd[i] == '\n' && i + 1 < nd.size()) line0.push_back(i + 1);
  const size_t nrows = line0.size();
  line0.push_back(nd.size());
  CHECK(nrows > 300, "the input has %zu rows: too few for the chunks", nrows);
  if (g_bad) return;
  const size_t cuts[] = {0, 1, 64, 128, 193, nrows};  // chunks of 1, 63, 64, 65 rows and the rest
  for (bool docs : {true, false}) {
    const char* what = docs ? "docs" : "no docs";
    Corpus W;
    flatten_ndjson(W, nd.data(), nd.size(), nsl.data(), nsl.size(), docs);
    CHECK((size_t)W.n == nrows, "%s: %lld rows flattened of %zu lines", what, (long long)W.n, nrows);
    std::vector<Corpus> src(5);
    std::vector<const Corpus*> sp;
    std::vector<uint64_t> all;
    for (size_t t = 0; t < 5; ++t) {
      const size_t a = line0[cuts[t]], b = line0[cuts[t + 1]];
      flatten_ndjson(src[t], nd.data() + a, b - a, nsl.data(), nsl.size(), docs);
      CHECK((size_t)src[t].n == cuts[t + 1] - cuts[t], "%s: chunk %zu has %lld rows", what, t, (long long)src[t].n);
      sp.push_back(&src[t]);
      for (size_t r = 0; r < cuts[t + 1] - cuts[t]; ++r) all.push_back(t), all.push_back(r);
    }
    if (g_bad) return;
    {
      Corpus G;
      gather_rows(G, sp, all.data(), all.size() / 2);
      same_columns(G, W, what);
    }
    // a shuffled subset, one pair twice; the same lines flattened afresh
    std::mt19937_64 rng(5);
    std::vector<std::pair<uint64_t, uint64_t>> sel;
    for (size_t k = 0; k < all.size() / 2; ++k)
      if (rng() % 5 != 0) sel.emplace_back(all[2 * k], all[2 * k + 1]);
    for (size_t k = sel.size(); k > 1; --k) std::swap(sel[k - 1], sel[rng() % k]);
    sel.push_back(sel[sel.size() / 2]);
    std::vector<uint64_t> pairs;
    std::string lines;
    for (const auto& p : sel) {
      pairs.push_back(p.first), pairs.push_back(p.second);
      const size_t row = cuts[p.first] + p.second;
      lines.append(nd, line0[row], line0[row + 1] - line0[row]);
      if (lines.empty() || lines.back() != '\n') lines += '\n';
    }
    Corpus G, F;
    gather_rows(G, sp, pairs.data(), sel.size());
    flatten_ndjson(F, lines.data(), lines.size(), nsl.data(), nsl.size(), docs);
    CHECK(G.n == F.n && (size_t)G.n == sel.size(), "%s subset: %lld rows gathered, %lld flattened", what, (long long)G.n, (long long)F.n);
    if (g_bad) return;
    std::vector<uint64_t> dg(G.n), df(F.n);
    row_digests(G, dg.data()), row_digests(F, df.data());
    std::vector<std::vector<uint64_t>> ds(5);
    for (size_t t = 0; t < 5; ++t) ds[t].resize(src[t].n), row_digests(src[t], ds[t].data());
    CHECK(ns_labels_json(G) == ns_labels_json(F), "%s subset: the label tables differ", what);
    CHECK(G.limit_rows == F.limit_rows, "%s subset: the rows past a limit differ", what);
    CHECK(G.hdr.size() == F.hdr.size(), "%s subset: the tile headers' count differs", what);
    bool moved = false;  // the id maps were not the identity: some row's namespace id differs from its source's
    for (size_t k = 0; k < sel.size(); ++k) {
      if (F.r_flags[k] & R_LIMIT) continue;  // equality is required of rows not past a limit
      CHECK(dg[k] == df[k], "%s subset: row %zu's digest differs from a fresh flatten's", what, k);
      CHECK(dg[k] == ds[sel[k].first][sel[k].second], "%s subset: row %zu's digest differs from its source row's", what, k);
      CHECK(G.r_flags[k] == F.r_flags[k], "%s subset: row %zu's flags", what, k);
      CHECK(G.dict[D_NS].at(G.r_nsa[k]) == F.dict[D_NS].at(F.r_nsa[k]), "%s subset: row %zu's namespace", what, k);
      moved = moved || G.r_nsa[k] != src[sel[k].first].r_nsa[sel[k].second];
    }
    CHECK(moved, "%s subset: every namespace id equals its source's: the id maps were not exercised", what);
  }
}

int main(int argc, char** argv) {
  if (argc != 1 && argc != 3) return fprintf(stderr, "usage: corpus_gather_check [<ndjson> <ns_labels_json>]\n"), 2;
  kernel_cases();
  if (argc == 3 && !g_bad) host_cases(slurp(argv[1]), slurp(argv[2]));
  if (g_bad) {
    fprintf(stderr, "corpus_gather_check: %d checks failed\n", g_bad);
    return 1;
  }
  printf("corpus_gather_check ok\n");
  return 0;
}
