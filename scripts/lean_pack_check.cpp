// Host check (ASan / UBSan) of the LEAN evaluation's compact container word and packed evidence
// numbering, from the functions the kernels and the host themselves call
// (kyverno_amd/csrc/kernels_abi.h):
//
//  (a) the container word (kpe_l6_pack_ctr, what kpe_lean_pack_kernel stores): for all 2^15
//      combinations of the used state bits, over a background of every unused CX_* bit set and
//      clear, the other bits of the CY word set and clear, and capability-set ids 0, 1, 2046 and
//      2047, the word unpacks to cx & KPE_L6_CX_USED and the id, has KPE_L6C_REAL and is not 0;
//  (b) the permutation kpe_l6_pack_ev: no two evidence bits share a packed bit, the packed clear
//      mask is the permuted KPE_L6_PT_CLR, the staged container word of the compact kernel is the
//      permuted staged word of the wide one;
//  (c) for every versioned check, the class masks and the pod table in the packed numbering
//      (what lean6_launch and kpe_device_open build for launches over the compact columns) give
//      the pass / fail of cv_fails, for every value of pod-word bits 0-22 with the tile check's
//      four container words, and for a stride of pod words with every one-bit word and its
//      complement. The in-place numbering is held to cv_fails by the same loop.
//
//   lean_pack_check        exits 0 when all hold, 2 with the first mismatch otherwise
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

#define CHECK(x, ...)                                                   \
  do {                                                                  \
    if (!(x)) {                                                         \
      fprintf(stderr, "lean_pack_check: %s (line %d): ", #x, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                                     \
      fprintf(stderr, "\n");                                            \
      exit(2);                                                          \
    }                                                                   \
  } while (0)

static void check_words() {
  CHECK(__builtin_popcount(KPE_L6_CX_USED) == (int)KPE_L6C_STATES, "used states %#x", KPE_L6_CX_USED);
  const uint32_t ids[4] = {0u, 1u, 2046u, 2047u};
  for (uint32_t s = 0; s < (1u << KPE_L6C_STATES); ++s) {
    const uint32_t used = kpe_l6_unpack_cx(s);
    CHECK((used & ~KPE_L6_CX_USED) == 0 && kpe_l6_pack_cx(used) == s, "states %#x in place %#x", s, used);
    for (uint32_t bg = 0; bg < 2u; ++bg)
      for (uint32_t hi = 0; hi < 2u; ++hi)
        for (uint32_t id : ids) {
          const uint32_t cx = used | (bg ? ~KPE_L6_CX_USED : 0u), cy = id | (hi ? 0xFFFF0000u : 0u);
          const uint32_t w = kpe_l6_pack_ctr(cx, cy);
          CHECK(w != 0 && (w & KPE_L6C_REAL), "cx %#x cy %#x word %#x", cx, cy, w);
          CHECK(kpe_l6_ctr_states(w) == (cx & KPE_L6_CX_USED), "states: cx %#x word %#x", cx, w);
          CHECK(kpe_l6_ctr_capset(w) == id, "id: cy %#x word %#x", cy, w);
          CHECK((w & ~(KPE_L6C_REAL | (KPE_L6C_ID_MASK << KPE_L6C_ID_SH) | ((1u << KPE_L6C_STATES) - 1u))) == 0,
                "stray bits: word %#x", w);
        }
  }
}

// every bit an in-place evidence word, class mask or table word can hold
static uint32_t evidence_bits() {
  uint32_t all = KPE_L6_CX_USED | (7u << KPE_L6_CAP_SH) | (1u << KPE_L6_SANN_SH) | KPE_L6_EV_SYS0 | KPE_L6_EV_SYS1 |
                 KPE_L6_EV_SYS2 | KPE_L6_EV_HOSTNS | (3u << KPE_L6_VOL_SH) | (3u << KPE_L6_ANN_SH) | KPE_L6_PT_NW;
  for (uint32_t cv = 0; cv < KPE_NUM_CV; ++cv) {
    bool nw;
    CHECK((kpe_l6_evidence(cv, &nw) & ~all) == 0, "check %u has evidence outside the known bits", cv);
  }
  return all;
}

static void check_permutation() {
  const uint32_t all = evidence_bits();
  uint32_t seen = 0;
  for (uint32_t b = 0; b < 32u; ++b) {
    const uint32_t p = kpe_l6_pack_ev(1u << b);
    if (!((all >> b) & 1u)) {
      CHECK(p == 0, "bit %u is no evidence bit but packs to %#x", b, p);
      continue;
    }
    CHECK(__builtin_popcount(p) == 1 && !(seen & p), "bit %u packs to %#x (taken %#x)", b, p, seen);
    seen |= p;
  }
  CHECK(kpe_l6_pack_ev(all) == seen && kpe_l6_pack_ev(KPE_L6_PT_NW) == KPE_L6_PT_NW, "packed bits %#x", seen);
  CHECK(kpe_l6_pack_ev(KPE_L6_PT_CLR) == KPE_L6C_PT_CLR, "clear mask %#x", kpe_l6_pack_ev(KPE_L6_PT_CLR));
  // the compact kernel's staged container word against the wide one's, permuted
  for (uint32_t s = 0; s < (1u << KPE_L6C_STATES); s += 7u)
    for (uint32_t code = 0; code < 8u; ++code)
      for (uint32_t sann = 0; sann < 2u; ++sann) {
        const uint32_t cx = kpe_l6_unpack_cx(s) | ~KPE_L6_CX_USED;
        const uint32_t wide = (cx & KPE_L6_CX_USED) | (code << KPE_L6_CAP_SH) | (sann << KPE_L6_SANN_SH);
        const uint32_t c = kpe_l6_pack_ctr(cx, 5u);
        const uint32_t comp = (c & ((1u << KPE_L6C_STATES) - 1u)) | (code << KPE_L6C_CAP_SH) | (sann << KPE_L6C_SANN_SH);
        CHECK(kpe_l6_pack_ev(wide) == comp, "staged word: states %#x code %u sann %u", s, code, sann);
      }
}

struct Tables {
  std::vector<uint32_t> tab, tab_c;  // exactly KPE_L6_PT_WORDS words each, on the heap
  KpeL6ClassMasks m[KPE_NUM_CV], m_c[KPE_NUM_CV];
};

// one pod word with one in-place word of container and list evidence, against cv_fails
static void check_one(const Tables& T, uint32_t pw, uint32_t cw) {
  const uint32_t xo = cw & KPE_L6_CX_USED, co = (cw >> KPE_L6_CAP_SH) & 7u, sann = (cw >> KPE_L6_SANN_SH) & 1u;
  const uint32_t vol = (cw >> KPE_L6_VOL_SH) & 3u, ann = (cw >> KPE_L6_ANN_SH) & 3u;
  const uint32_t sys = ((cw & KPE_L6_EV_SYS0) ? 1u : 0u) | ((cw & KPE_L6_EV_SYS1) ? 2u : 0u) | ((cw & KPE_L6_EV_SYS2) ? 4u : 0u);
  const uint32_t want = cv_fails(pw, xo, co, sann != 0u, (vol & 1u) != 0u, (vol & 2u) != 0u, sys, (ann & 1u) != 0u, (ann & 2u) != 0u);
  // in place, as the wide verdict-only form computes it
  const uint32_t sys_ev = ((sys & 3u) << 1) | ((sys & 4u) << 2);
  const uint32_t tw = kpe_l6_pod_lookup(T.tab.data(), pw);
  const uint32_t ev = kpe_l6_pod_split(xo | (co << KPE_L6_CAP_SH) | (sann << KPE_L6_SANN_SH), tw,
                                       (vol << KPE_L6_VOL_SH) | sys_ev | (ann << KPE_L6_ANN_SH));
  const uint32_t ev_nw = ev & (uint32_t)((int32_t)tw >> 31);
  // packed, as the compact form does
  const uint32_t twc = kpe_l6_pod_lookup(T.tab_c.data(), pw);
  const uint32_t evc = kpe_l6c_pod_split(kpe_l6_pack_cx(xo) | (co << KPE_L6C_CAP_SH) | (sann << KPE_L6C_SANN_SH), twc,
                                         (vol << KPE_L6C_VOL_SH) | (sys << KPE_L6C_SYS_SH) | (ann << KPE_L6C_ANN_SH));
  const uint32_t evc_nw = evc & (uint32_t)((int32_t)twc >> 31);
  CHECK(evc == kpe_l6_pack_ev(ev), "evidence: pw %#x cw %#x packed %#x in place %#x", pw, cw, evc, ev);
  uint32_t got = 0, got_c = 0;
  for (uint32_t cv = 0; cv < KPE_NUM_CV; ++cv) {
    const KpeL6ClassMasks &m = T.m[cv], &mc = T.m_c[cv];
    if ((ev & m.ev) | (ev_nw & m.ev_nw)) got |= 1u << cv;
    if ((evc & mc.ev) | (evc_nw & mc.ev_nw)) got_c |= 1u << cv;
  }
  CHECK(got == want, "in place: pw %#x cw %#x fails %#x cv_fails %#x", pw, cw, got, want);
  CHECK(got_c == want, "packed: pw %#x cw %#x fails %#x cv_fails %#x", pw, cw, got_c, want);
}

static void check_verdicts() {
  Tables T;
  T.tab.resize(KPE_L6_PT_WORDS), T.tab_c.resize(KPE_L6_PT_WORDS);
  for (uint32_t i = 0; i < KPE_L6_PT_WORDS; ++i) T.tab[i] = kpe_l6_pod_table_word(i), T.tab_c[i] = kpe_l6_pack_ev(T.tab[i]);
  for (uint32_t cv = 0; cv < KPE_NUM_CV; ++cv) {
    T.m[cv] = kpe_l6_class_masks(1u << cv);
    T.m_c[cv] = KpeL6ClassMasks{kpe_l6_pack_ev(T.m[cv].ev), kpe_l6_pack_ev(T.m[cv].ev_nw)};
  }
  const uint32_t lists = evidence_bits() & ~(KPE_L6_EV_HOSTNS | KPE_L6_PT_NW);  // what containers and lists may set
  const uint32_t cws[4] = {0u, ~0u, 0x55555555u, 0xAAAAAAAAu};
  for (uint32_t pw = 0; pw < (1u << 23); ++pw)
    for (uint32_t cw : cws) check_one(T, pw, cw & lists);
  for (uint32_t pw = 0; pw < (1u << 23); pw += 4099u)
    for (uint32_t b = 0; b < 32u; ++b) {
      check_one(T, pw, (1u << b) & lists);
      check_one(T, pw, ~(1u << b) & lists);
    }
}

int main() {
  check_words();
  check_permutation();
  check_verdicts();
  printf("lean_pack_check ok\n");
  return 0;
}
