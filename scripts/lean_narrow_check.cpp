// Host check (ASan / UBSan) of the LEAN evaluation's pod word column pw4, from the functions the
// kernels and the host themselves call (kyverno_amd/csrc/kernels_abi.h kpe_l6_pack_pod,
// kpe_l6p_*): what the narrow scatter form reads of a pod must be what the rec12 form reads of it.
//
// For every x in 0 .. 2^23 - 1 (every bit the evaluation reads of the pod word, and bit 0, which
// it does not) and the kind ids 0, 1, 511 and 1023, over a background of bits 23-31 of x and the
// version / group bits of y clear and set:
//
//  (a) kpe_l6p_pod_lookup of the packed word equals kpe_l6_pod_lookup of x, over the table the
//      kernel reads (the packed numbering) and over one whose every entry is distinct, so a wrong
//      index cannot hide behind equal entries;
//  (b) the class, the decode error and the kind id come back;
//  (c) the packed word does not depend on the background: nothing of bits 23-31 of x or of the
//      version and group of y leaks in.
//
//   lean_narrow_check        exits 0 when all hold, 2 with the first mismatch otherwise
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct uint2 {  // the HIP vector types kernels_abi.h names
  uint32_t x, y;
};
struct uint4 {
  uint32_t x, y, z, w;
};
#include "../kyverno_amd/csrc/kernels_abi.h"

#define CHECK(x, ...)                                                     \
  do {                                                                    \
    if (!(x)) {                                                           \
      fprintf(stderr, "lean_narrow_check: %s (line %d): ", #x, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                                       \
      fprintf(stderr, "\n");                                              \
      exit(2);                                                            \
    }                                                                     \
  } while (0)

int main() {
  std::vector<uint32_t> tab_c(KPE_L6_PT_WORDS), tab_d(KPE_L6_PT_WORDS);
  for (uint32_t i = 0; i < KPE_L6_PT_WORDS; ++i) {
    tab_c[i] = kpe_l6_pack_ev(kpe_l6_pod_table_word(i));
    // one bit group per slice and a distinct value per entry: the OR of three entries names all three
    tab_d[i] = i < KPE_L6_PT_B0 ? i : i < KPE_L6_PT_C0 ? (i - KPE_L6_PT_B0) << 7 : (i - KPE_L6_PT_C0) << 15;
  }
  const uint32_t kinds[4] = {0u, 1u, 511u, 1023u};
  const uint32_t xbg = ~((1u << 23) - 1u), ybg = ~0xFFFu;
  for (uint32_t x = 0; x < (1u << 23); ++x) {
    const uint32_t cls = (x >> PR_CLASS_SH) & R_CLASS_MASK, derr = (x & PR_DECODE_ERR) ? 1u : 0u;
    const uint32_t want_c = kpe_l6_pod_lookup(tab_c.data(), x), want_d = kpe_l6_pod_lookup(tab_d.data(), x);
    for (uint32_t kind : kinds) {
      const uint32_t w = kpe_l6_pack_pod(x, kind);
      CHECK(kpe_l6p_pod_lookup(tab_c.data(), w) == want_c, "lookup: x %#x word %#x", x, w);
      CHECK(kpe_l6p_pod_lookup(tab_d.data(), w) == want_d, "lookup (distinct entries): x %#x word %#x", x, w);
      CHECK(kpe_l6p_class(w) == cls, "class: x %#x word %#x", x, w);
      CHECK(((w & KPE_L6P_DECODE_ERR) ? 1u : 0u) == derr, "decode error: x %#x word %#x", x, w);
      CHECK(kpe_l6p_kind(w) == kind, "kind %u: x %#x word %#x", kind, x, w);
      CHECK(kpe_l6_pack_pod(x | xbg, kind | ybg) == w, "bits 23-31 of x / version and group of y leak: x %#x kind %u", x, kind);
      CHECK(kpe_l6_pack_pod(x | xbg, kind) == w && kpe_l6_pack_pod(x, kind | ybg) == w, "background: x %#x kind %u", x, kind);
    }
  }
  // bit 0 of x (P_SC_PRESENT) is no input of the table either
  CHECK(kpe_l6_pack_pod(1u, 0u) == 0u, "bit 0 of x");
  printf("lean_narrow_check ok\n");
  return 0;
}
