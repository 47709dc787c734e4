// Host check (ASan / UBSan) of the pieces of kpe_lean6_kernel's tile body that can go wrong
// silently, from the functions the kernel itself calls (kyverno_amd/csrc/kernels_abi.h):
//
//  (a) the pod-evidence table against the field logic, for every value of pod-word bits 0-22
//      (8.4M words): the table word's set bits, clear bits and not-Windows flag, and the evidence
//      word it gives with container words that have all, none and alternating bits;
//  (b) the four-word container read against a loop over the pod's slots, for every first slot and
//      count of a stage laid out as the kernel's (128 words, then the byte arrays), over a buffer
//      of exactly the stage's size: a read past it is a sanitizer report;
//  (c) the class masks the host builds (kpe_l6_class_masks, the function lean6_launch calls): for
//      every versioned check and pair of checks, the kernel's test equals the rule of
//      kpe_l6_evidence for every evidence bit, Windows pod or not.
//
//   lean_tile_check        exits 0 when all hold, 2 with the first mismatch otherwise
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct uint2 {  // the HIP vector types kernels_abi.h names
  uint32_t x, y;
};
struct uint4 {
  uint32_t x, y, z, w;
};
#include "../kyverno_amd/csrc/kernels_abi.h"

#define CHECK(x, ...)                                                   \
  do {                                                                  \
    if (!(x)) {                                                         \
      fprintf(stderr, "lean_tile_check: %s (line %d): ", #x, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                                     \
      fprintf(stderr, "\n");                                            \
      exit(2);                                                          \
    }                                                                   \
  } while (0)

static void check_table() {
  // exactly KPE_L6_PT_WORDS words on the heap: an index past a slice is a sanitizer report
  std::vector<uint32_t> tab(KPE_L6_PT_WORDS);
  for (uint32_t i = 0; i < KPE_L6_PT_WORDS; ++i) tab[i] = kpe_l6_pod_table_word(i);
  const uint32_t cws[4] = {0u, ~0u, 0x55555555u, 0xAAAAAAAAu};
  for (uint32_t pw = 0; pw < (1u << 23); ++pw) {
    uint32_t set, clr;
    kpe_l6_pod_evidence(pw, &set, &clr);
    CHECK((set & (KPE_L6_PT_CLR | KPE_L6_PT_NW)) == 0 && (clr & ~KPE_L6_PT_CLR) == 0, "pw %#x", pw);
    const uint32_t tw = kpe_l6_pod_lookup(tab.data(), pw);
    CHECK((tw & ~(KPE_L6_PT_CLR | KPE_L6_PT_NW)) == set, "set: pw %#x table %#x logic %#x", pw, tw, set);
    CHECK((tw & KPE_L6_PT_CLR) == clr, "clr: pw %#x table %#x logic %#x", pw, tw, clr);
    const uint32_t nwin = (uint32_t)((int32_t)tw >> 31);  // as the kernel spreads the flag
    CHECK(nwin == (kpe_l6_not_windows(pw) ? ~0u : 0u), "nwin: pw %#x table %#x", pw, tw);
    for (uint32_t cw : cws) {
      const uint32_t lists = cw & ((3u << KPE_L6_VOL_SH) | (3u << KPE_L6_ANN_SH) | KPE_L6_EV_SYS0 | KPE_L6_EV_SYS2);
      CHECK(kpe_l6_pod_split(cw, tw, lists) == ((cw & ~clr) | set | lists), "split: pw %#x cw %#x", pw, cw);
    }
  }
}

static void check_containers() {
  // the wave's stage: KPE_L6_CTR words, then the byte arrays (kernels_abi.h KPE_L6_STAGE_BYTES)
  uint32_t* stage = static_cast<uint32_t*>(malloc(KPE_L6_STAGE_BYTES));
  CHECK(stage, "malloc");
  uint32_t x = 0x9E3779B9u;
  for (uint32_t i = 0; i < KPE_L6_STAGE_BYTES / 4u; ++i) stage[i] = (x = x * 1664525u + 1013904223u);
  for (uint32_t oc = 0; oc < 300u; ++oc)  // offsets past the stage: the kernel clamps the address
    for (uint32_t nc = 0; nc <= 4u; ++nc) {
      const uint32_t* p = stage + (oc < KPE_L6_CTR - 1u ? oc : KPE_L6_CTR - 1u);
      const uint32_t got = kpe_l6_ctr_or(p[0], p[1], p[2], p[3], nc);
      if (oc + nc > KPE_L6_CTR) continue;  // recomputed by the kernel's slow path
      uint32_t want = 0;
      for (uint32_t k = oc; k < oc + nc; ++k) want |= stage[k];
      CHECK(got == want, "containers: slot %u count %u", oc, nc);
    }
  free(stage);
}

static void check_classes() {
  // Every versioned check alone and every pair, through the function lean6_launch fills
  // LeanBatchArgs::cls_ev / cls_ev_nw with: the kernel's test (ev & nwin computed once, two ANDs
  // per class) against the rule "some bit of kpe_l6_evidence(cv) is set, and the pod is not a
  // Windows pod if the check spares those", for every single evidence bit.
  for (uint32_t c1 = 0; c1 < KPE_NUM_CV; ++c1)
    for (uint32_t c2 = c1; c2 < KPE_NUM_CV; ++c2) {
      const uint32_t checks = (1u << c1) | (1u << c2);
      const KpeL6ClassMasks m = kpe_l6_class_masks(checks);
      for (uint32_t b = 0; b < 32u; ++b)
        for (uint32_t win = 0; win < 2u; ++win) {
          const uint32_t ev = 1u << b, nwin = win ? 0u : ~0u;
          bool want = false;
          for (uint32_t cv : {c1, c2}) {
            bool nw;
            const uint32_t bits = kpe_l6_evidence(cv, &nw);
            want = want || (((bits >> b) & 1u) && !(nw && win));
          }
          const uint32_t ev_nw = ev & nwin;
          const bool got = ((ev & m.ev) | (ev_nw & m.ev_nw)) != 0;
          CHECK(got == want, "class: checks %#x bit %u windows %u", checks, b, win);
        }
    }
}

int main() {
  check_table();
  check_containers();
  check_classes();
  printf("lean_tile_check ok\n");
  return 0;
}
