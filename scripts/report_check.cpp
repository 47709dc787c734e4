// Host run of the report renderer (kyverno_amd/csrc/report.cpp, the text libkpe.so is built from)
// under ASan / UBSan, with the flattener and the compiler and without the HIP runtime: the program
// and corpus handles are built here through api_internal.h's host part, every row is rendered with
// its resource JSON by the per-row call (kpe_report_results_msg_tr, no traces), then all rows by
// the bulk call (kpe_report_results_rows over kpe_report_cells_host's sparse mask list) with
// KPE_REPORT_THREADS at 1 and at 4.
//
//   report_check <policies.json> <resources.ndjson> <rows.bin> <texts-out>
// rows.bin: u64 nrows, u64 R, u8 verdicts[nrows R], u32 cv_masks[nrows R] (the kpe_fetch_cv_masks
// layout); row k is the k-th non-empty line of the NDJSON. Writes u64 nrows, u64 offsets[nrows + 1],
// then the per-row texts; exits non-zero when a bulk rendering differs from them
// (tests/test_report.py compares the texts with libkpe.so's).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../kyverno_amd/csrc/api_internal.h"

#define CHECK(x)                                                     \
  do {                                                               \
    if (!(x)) {                                                      \
      fprintf(stderr, "report_check: %s (line %d)\n", #x, __LINE__); \
      exit(2);                                                       \
    }                                                                \
  } while (0)

namespace kpe {
void flatten_ndjson(Corpus& C, const char* buf, size_t len, const char* nsl, size_t nsl_len, bool docs);
// what kpe_api.cpp defines for the library: the error text's sink, and the end of a corpus handle
// (no handle of this program has a device half)
struct DeviceCorpus {};
kpe_status fail(kpe_status s, const std::string& m) {
  fprintf(stderr, "report_check: status %d: %s\n", (int)s, m.c_str());
  return s;
}
}  // namespace kpe
kpe_corpus::~kpe_corpus() = default;

static std::string slurp(const char* path) {
  FILE* f = fopen(path, "rb");
  CHECK(f);
  std::string s;
  char buf[1 << 16];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) s.append(buf, n);
  fclose(f);
  return s;
}

int main(int argc, char** argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: %s policies.json resources.ndjson rows.bin texts-out\n", argv[0]);
    return 2;
  }
  const std::string pj = slurp(argv[1]), nd = slurp(argv[2]), rb = slurp(argv[3]);
  kpe_program prog{kpe::compile_policies(pj.data(), pj.size())};
  kpe_corpus corpus{std::make_unique<kpe::Corpus>(), nullptr};
  kpe::flatten_ndjson(*corpus.c, nd.data(), nd.size(), nullptr, 0, true);

  std::vector<const char*> res;
  std::vector<size_t> res_len;
  for (size_t b = 0; b < nd.size();) {
    const char* nl = static_cast<const char*>(memchr(nd.data() + b, '\n', nd.size() - b));
    const size_t e = nl ? (size_t)(nl - nd.data()) : nd.size();
    if (e > b) res.push_back(nd.data() + b), res_len.push_back(e - b);
    b = e + 1;
  }
  uint64_t hdr[2];
  CHECK(rb.size() >= sizeof hdr);
  memcpy(hdr, rb.data(), sizeof hdr);
  const uint64_t nrows = hdr[0], R = hdr[1];
  CHECK(R == prog.p->rules.size() && nrows == res.size() && nrows == (uint64_t)corpus.c->n);
  CHECK(rb.size() == sizeof hdr + nrows * R * 5);
  // exact-size heap copies: a read past a row is a sanitizer report
  std::vector<uint8_t> v(nrows * R);
  std::vector<uint32_t> m(nrows * R);
  memcpy(v.data(), rb.data() + sizeof hdr, v.size());
  memcpy(m.data(), rb.data() + sizeof hdr + v.size(), m.size() * 4);

  std::vector<std::string> want(nrows);
  for (uint64_t k = 0; k < nrows; ++k) {
    const long n = kpe_report_results_msg_tr(&prog, &corpus, v.data() + k * R, m.data() + k * R, nullptr, res[k],
                                             res_len[k], nullptr, 0);
    CHECK(n >= 0);
    std::vector<char> buf((size_t)n + 1);
    CHECK(kpe_report_results_msg_tr(&prog, &corpus, v.data() + k * R, m.data() + k * R, nullptr, res[k], res_len[k],
                                    buf.data(), buf.size()) == n);
    want[k].assign(buf.data(), (size_t)n);
    CHECK(buf[(size_t)n] == 0);
  }

  // the bulk call's input: the mask words of the cells the renderer reads, a count call then an exact one
  kpe_report_rows io{};
  CHECK(kpe_report_cells_host(&prog, nrows, v.data(), m.data(), nullptr, KPE_RR_MASKS, &io) == KPE_OK);
  std::vector<uint64_t> cells(io.mask_total);
  std::vector<uint32_t> words(io.mask_total);
  io.verdict_rows = v.data();
  io.mask_cells = cells.data(), io.mask_words = words.data(), io.mask_cap = io.mask_total;
  CHECK(kpe_report_cells_host(&prog, nrows, v.data(), m.data(), nullptr, KPE_RR_MASKS, &io) == KPE_OK);
  CHECK(io.mask_total == cells.size());
  int bad = 0;
  for (const char* threads : {"1", "4"}) {
    setenv("KPE_REPORT_THREADS", threads, 1);
    std::vector<uint64_t> off(nrows + 1);
    const long n = kpe_report_results_rows(&prog, &corpus, nrows, &io, res.data(), res_len.data(), nullptr, 0, off.data());
    CHECK(n >= 0);
    std::vector<char> buf((size_t)n + 1);
    CHECK(kpe_report_results_rows(&prog, &corpus, nrows, &io, res.data(), res_len.data(), buf.data(), buf.size(),
                                  off.data()) == n);
    CHECK(off[nrows] == (uint64_t)n);
    for (uint64_t k = 0; k < nrows; ++k)
      if (std::string(buf.data() + off[k], off[k + 1] - off[k]) != want[k]) {
        if (!bad++) fprintf(stderr, "report_check: row %llu differs with %s thread(s)\n", (unsigned long long)k, threads);
      }
  }

  FILE* f = fopen(argv[4], "wb");
  CHECK(f);
  uint64_t o = 0;
  CHECK(fwrite(&nrows, 8, 1, f) == 1);
  for (uint64_t k = 0; k <= nrows; ++k) {
    CHECK(fwrite(&o, 8, 1, f) == 1);
    if (k < nrows) o += want[k].size();
  }
  for (const std::string& t : want) CHECK(t.empty() || fwrite(t.data(), 1, t.size(), f) == t.size());
  CHECK(fclose(f) == 0);
  return bad ? 1 : 0;
}
