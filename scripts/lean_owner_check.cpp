// Host check (ASan / UBSan) of the LEAN evaluation's owner-tagged columns and of the scatter that
// reads them, from the functions the kernels and the host themselves call
// (kyverno_amd/csrc/kernels_abi.h kpe_l6_tag_*):
//
//  (a) the container word (kpe_l6_tag_ctr, what kpe_lean_tag_kernel stores) unpacks to its used
//      states, capability-set id and owner, for all 2^15 state combinations, all 64 owners and
//      ids 0 and 2047, over a background of every other CX_* / CY bit set and clear; the sysctl /
//      annotation-key word to its id and owner, and KPE_NO_STR stays past every dictionary size
//      the tagged columns are built for;
//  (b) the volume word: for the mask 0 and all 29 single-source masks kpe_l6_vol_decide gives
//      vol_code of the mask and the word has no escape flag; every two-source mask of a fixed list
//      (and a few of more sources) has it;
//  (c) a plain C++ model of the tile body, "mask by the tile's count, OR into acc[owner]", with the
//      kernel's slot pattern (128 containers and volumes, 64 sysctls and annotations, then batches
//      of 64; slots past a tile's count hold the next tile's items, whose owners alias this
//      tile's pods, or the next column, or slack) over hand-built tiles: the evidence word of
//      every pod, taken through the packed class masks and pod table, fails exactly the versioned
//      checks that cv_fails gives for the per-pod OR of kpe_l6_ctr_states and the list codes.
//
//   lean_owner_check        exits 0 when all hold, 2 with the first mismatch otherwise
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

#define CHECK(x, ...)                                                    \
  do {                                                                   \
    if (!(x)) {                                                          \
      fprintf(stderr, "lean_owner_check: %s (line %d): ", #x, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                                      \
      fprintf(stderr, "\n");                                             \
      exit(2);                                                           \
    }                                                                    \
  } while (0)

static uint32_t vol_code(uint32_t v) { return ((v >> VS_HOSTPATH) & 1u) | ((v & PSS_ALLOWED_VOLUMES) ? 0u : 2u); }

static void check_words() {
  const uint32_t ids[2] = {0u, 2047u};
  for (uint32_t s = 0; s < (1u << KPE_L6C_STATES); ++s) {
    const uint32_t used = kpe_l6_unpack_cx(s);
    for (uint32_t owner = 0; owner < 64u; ++owner)
      for (uint32_t id : ids) {
        const uint32_t bg = (s ^ owner) & 1u;  // the unused bits set for half of the words
        const uint32_t cx = used | (bg ? ~KPE_L6_CX_USED : 0u), cy = id | (bg ? 0xFFFF0000u : 0u);
        const uint32_t w = kpe_l6_tag_ctr(cx, cy, owner);
        CHECK(kpe_l6_ctr_states(w) == used, "states: cx %#x owner %u word %#x", cx, owner, w);
        CHECK(kpe_l6_ctr_capset(w) == id, "id: cy %#x owner %u word %#x", cy, owner, w);
        CHECK(kpe_l6_tag_owner(w) == owner, "owner %u word %#x", owner, w);
      }
  }
  const uint32_t sids[5] = {0u, 1u, 12345u, KPE_L6T_ID_MASK - 1u, KPE_NO_STR};
  for (uint32_t owner = 0; owner < 64u; ++owner)
    for (uint32_t id : sids) {
      const uint32_t w = kpe_l6_tag_id(id, owner);
      CHECK(kpe_l6_tag_owner(w) == owner && kpe_l6_tag_get_id(w) == (id & KPE_L6T_ID_MASK), "id %#x owner %u word %#x", id,
            owner, w);
    }
  // a masked KPE_NO_STR is no id of a dictionary the tagged columns are built for (< KPE_L6T_ID_MASK entries)
  CHECK(kpe_l6_tag_get_id(kpe_l6_tag_id(KPE_NO_STR, 63u)) >= KPE_L6T_ID_MASK, "KPE_NO_STR masks to an id");
}

static void check_volumes() {
  for (uint32_t owner = 0; owner < 64u; owner += 21u) {
    const uint32_t w0 = kpe_l6_tag_vol(0u, owner);
    CHECK(!(w0 & KPE_L6T_VOL_ESC) && kpe_l6_vol_decide(w0) == vol_code(0u), "no source: %#x", w0);
    CHECK(kpe_l6_tag_owner(w0) == owner, "owner %u word %#x", owner, w0);
    for (uint32_t b = 0; b <= VS_EPHEMERAL; ++b) {
      const uint32_t w = kpe_l6_tag_vol(1u << b, owner);
      CHECK(!(w & KPE_L6T_VOL_ESC) && (w & KPE_L6T_VOL_IDX) == b, "source %u: word %#x", b, w);
      CHECK(kpe_l6_vol_decide(w) == vol_code(1u << b), "source %u: %u, vol_code %u", b, kpe_l6_vol_decide(w), vol_code(1u << b));
      CHECK(kpe_l6_tag_owner(w) == owner, "owner %u word %#x", owner, w);
    }
    const uint32_t multi[] = {(1u << VS_HOSTPATH) | (1u << VS_EMPTYDIR),  (1u << VS_EMPTYDIR) | (1u << VS_CONFIGMAP),
                              (1u << VS_HOSTPATH) | (1u << VS_EPHEMERAL), (1u << VS_NFS) | (1u << VS_SECRET),
                              (1u << VS_CSI) | (1u << VS_EPHEMERAL),      (1u << VS_GCEPD) | (1u << VS_AWSEBS),
                              (1u << VS_PVC) | (1u << VS_PROJECTED),      7u, 0x1FFFFFFFu};
    for (uint32_t m : multi) {
      const uint32_t w = kpe_l6_tag_vol(m, owner);
      CHECK((w & KPE_L6T_VOL_ESC) && kpe_l6_tag_owner(w) == owner, "sources %#x: word %#x", m, w);
    }
  }
}

// ---- (c) the scatter over hand-built tiles ----
struct Pod {
  uint32_t pw;
  std::vector<uint2> ctr;     // {cx, cy}
  std::vector<uint32_t> vol;  // source masks
  std::vector<uint32_t> sys;  // ids
  std::vector<uint2> ann;     // {key id, value id}
};
// code tables a corpus could have (any function of the id will do: both sides read the same one)
static uint32_t cap_code(uint32_t id) { return (id * 5u + 3u) & 7u; }
static uint32_t sys_code(uint32_t id) { return id == (KPE_NO_STR & KPE_L6T_ID_MASK) ? 7u : (id * 3u) & 7u; }
static uint32_t ann_code(uint2 q) { return (q.x ^ (q.y >> 1)) & 3u; }

struct Tables {
  std::vector<uint32_t> tab_c;
  KpeL6ClassMasks m_c[KPE_NUM_CV];
};

static uint32_t rnd(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

static void check_scatter(const std::vector<Pod>& pods, const Tables& T, const char* what) {
  const size_t n = pods.size(), ntiles = (n + 63) / 64;
  // the columns as kpe_lean_tag_kernel lays them out: one allocation, zeroed, then every item
  // with its owner
  size_t nctr = 0, nvol = 0, nsys = 0, nann = 0;
  for (const Pod& p : pods) nctr += p.ctr.size(), nvol += p.vol.size(), nsys += p.sys.size(), nann += p.ann.size();
  const KpeL6TagLayout lay = kpe_l6_tag_layout((uint32_t)nctr, (uint32_t)nvol, (uint32_t)nsys, (uint32_t)nann);
  std::vector<uint32_t> tag(lay.bytes / 4, 0u), vsrc;
  std::vector<uint32_t> hdr(4 * (ntiles + 1));
  {
    size_t c = 0, v = 0, s = 0, a = 0;
    for (size_t r = 0; r < n; ++r) {
      if (!(r & 63)) hdr[4 * (r >> 6)] = (uint32_t)c, hdr[4 * (r >> 6) + 1] = (uint32_t)v, hdr[4 * (r >> 6) + 2] = (uint32_t)s, hdr[4 * (r >> 6) + 3] = (uint32_t)a;
      const uint32_t o = (uint32_t)(r & 63);
      for (const uint2& e : pods[r].ctr) tag[c++] = kpe_l6_tag_ctr(e.x, e.y, o);
      for (uint32_t m : pods[r].vol) tag[lay.o_vol / 4 + v++] = kpe_l6_tag_vol(m, o), vsrc.push_back(m);
      for (uint32_t id : pods[r].sys) tag[lay.o_sys / 4 + s++] = kpe_l6_tag_id(id, o);
      for (const uint2& q : pods[r].ann) tag[lay.o_ann / 4 + 2 * a] = kpe_l6_tag_id(q.x, o), tag[lay.o_ann / 4 + 2 * a + 1] = q.y, ++a;
    }
    hdr[4 * ntiles] = (uint32_t)c, hdr[4 * ntiles + 1] = (uint32_t)v, hdr[4 * ntiles + 2] = (uint32_t)s, hdr[4 * ntiles + 3] = (uint32_t)a;
  }
  auto word = [&](uint64_t byte) -> uint32_t {
    CHECK(byte + 4 <= lay.bytes, "%s: a load at byte %llu of %llu", what, (unsigned long long)byte, (unsigned long long)lay.bytes);
    return tag[byte / 4];
  };
  for (size_t t = 0; t < ntiles; ++t) {
    const uint32_t* h = &hdr[4 * t];
    const uint32_t nct = h[4] - h[0], nvt = h[5] - h[1], nst = h[6] - h[2], nat = h[7] - h[3];
    uint32_t acc[64];
    memset(acc, 0, sizeof acc);
    // slot s of a list, loaded whether or not it is an item of the tile, ORed under the count
    auto slots = [](uint32_t first, uint32_t count) { return count <= first ? first : first + ((count - first + 63u) / 64u) * 64u; };
    for (uint32_t s = 0; s < slots(KPE_L6_CTR, nct); ++s) {
      const uint32_t e = word(4ull * (h[0] + s));
      const uint32_t ev = (e & ((1u << KPE_L6C_STATES) - 1u)) | (cap_code(kpe_l6_ctr_capset(e)) << KPE_L6C_CAP_SH);
      acc[kpe_l6_tag_owner(e)] |= s < nct ? ev : 0u;
    }
    for (uint32_t s = 0; s < slots(KPE_L6_VOL, nvt); ++s) {
      const uint32_t w = word(lay.o_vol + 4ull * (h[1] + s));
      uint32_t c = kpe_l6_vol_decide(w);
      if (s < nvt && (w & KPE_L6T_VOL_ESC)) c = vol_code(vsrc[h[1] + s]);
      acc[kpe_l6_tag_owner(w)] |= s < nvt ? c << KPE_L6C_VOL_SH : 0u;
    }
    for (uint32_t s = 0; s < slots(KPE_L6_SMALL, nst); ++s) {
      const uint32_t w = word(lay.o_sys + 4ull * (h[2] + s));
      acc[kpe_l6_tag_owner(w)] |= s < nst ? sys_code(kpe_l6_tag_get_id(w)) << KPE_L6C_SYS_SH : 0u;
    }
    for (uint32_t s = 0; s < slots(KPE_L6_SMALL, nat); ++s) {
      const uint32_t k = word(lay.o_ann + 8ull * (h[3] + s)), v = word(lay.o_ann + 8ull * (h[3] + s) + 4);
      acc[kpe_l6_tag_owner(k)] |= s < nat ? ann_code(uint2{kpe_l6_tag_get_id(k), v}) << KPE_L6C_ANN_SH : 0u;
    }
    for (size_t r = 64 * t; r < n && r < 64 * (t + 1); ++r) {
      const Pod& p = pods[r];
      uint32_t xo = 0, co = 0, vc = 0, sc = 0, ac = 0;
      for (const uint2& e : p.ctr) {
        const uint32_t w = kpe_l6_pack_ctr(e.x, e.y);
        xo |= kpe_l6_ctr_states(w), co |= cap_code(kpe_l6_ctr_capset(w));
      }
      for (uint32_t m : p.vol) vc |= vol_code(m);
      for (uint32_t id : p.sys) sc |= sys_code(id & KPE_L6T_ID_MASK);
      for (const uint2& q : p.ann) ac |= ann_code(uint2{q.x & KPE_L6T_ID_MASK, q.y});
      const uint32_t want = cv_fails(p.pw, xo, co, false, (vc & 1u) != 0u, (vc & 2u) != 0u, sc, (ac & 1u) != 0u, (ac & 2u) != 0u);
      const uint32_t tw = kpe_l6_pod_lookup(T.tab_c.data(), p.pw);
      const uint32_t ev = kpe_l6c_pod_split(acc[r & 63], tw, 0u);
      const uint32_t ev_nw = ev & (uint32_t)((int32_t)tw >> 31);
      uint32_t got = 0;
      for (uint32_t cv = 0; cv < KPE_NUM_CV; ++cv)
        if ((ev & T.m_c[cv].ev) | (ev_nw & T.m_c[cv].ev_nw)) got |= 1u << cv;
      CHECK(got == want, "%s: row %zu evidence %#x fails %#x cv_fails %#x", what, r, ev, got, want);
    }
  }
}

static Pod clean_pod() { return Pod{0u, {uint2{0u, 1u}}, {1u << VS_EMPTYDIR}, {}, {}}; }

static void check_tiles() {
  Tables T;
  T.tab_c.resize(KPE_L6_PT_WORDS);
  for (uint32_t i = 0; i < KPE_L6_PT_WORDS; ++i) T.tab_c[i] = kpe_l6_pack_ev(kpe_l6_pod_table_word(i));
  for (uint32_t cv = 0; cv < KPE_NUM_CV; ++cv) {
    const KpeL6ClassMasks m = kpe_l6_class_masks(1u << cv);
    T.m_c[cv] = KpeL6ClassMasks{kpe_l6_pack_ev(m.ev), kpe_l6_pack_ev(m.ev_nw)};
  }
  // each used state bit in turn, as a CX word
  std::vector<uint32_t> bits;
  for (uint32_t b = 0; b < 32u; ++b)
    if ((KPE_L6_CX_USED >> b) & 1u) bits.push_back(1u << b);
  {  // tile A with few items and no finding; tile B's first pods offend in every list: A's slack
    // slots hold B's items, whose owners 0, 1, 2, ... are A's pods
    std::vector<Pod> pods;
    for (uint32_t r = 0; r < 64u; ++r) {
      Pod p = clean_pod();
      if (r % 3u == 0u) p.ctr.clear(), p.vol.clear();  // pods with no item of any list
      // a few clean sysctls and annotations (code 0): A's counts are 21, and slot [count] of each
      // list holds B's first, offending item, whose owner 0 is A's first pod
      if (r % 3u == 1u) p.sys = {0u}, p.ann = {uint2{0u, 0u}};
      pods.push_back(p);
    }
    for (uint32_t r = 0; r < 65u; ++r) {
      Pod p = clean_pod();
      if (r < 20u) {
        p.ctr = {uint2{bits[r % bits.size()], 2047u}, uint2{KPE_L6_CX_USED, 7u}};
        p.vol = {1u << VS_HOSTPATH, (1u << VS_HOSTPATH) | (1u << VS_EMPTYDIR), 0u};
        p.sys = {5u, KPE_NO_STR};
        p.ann = {uint2{1u, 0u}, uint2{2u, KPE_NO_STR}};
      }
      pods.push_back(p);
    }
    check_scatter(pods, T, "few then offending");
  }
  {  // one pod of 200 containers among clean ones, the offender at each position in turn; and full
    // batches of volumes, sysctls and annotations
    for (uint32_t at : {0u, 63u, 64u, 127u, 128u, 191u, 199u}) {
      std::vector<Pod> pods;
      for (uint32_t r = 0; r < 70u; ++r) pods.push_back(clean_pod());
      pods[9].ctr.assign(200, uint2{0u, 1u});
      pods[9].ctr[at] = uint2{bits[at % bits.size()], 3u};
      for (uint32_t r = 0; r < 64u; ++r) {
        pods[r].vol.assign(3, 1u << VS_SECRET);
        pods[r].sys.assign(2, 0u);
        pods[r].ann.assign(2, uint2{0u, 0u});
        if (r % 5u == 0u) {
          pods[r].vol[(r / 5u) % 3u] = 1u << VS_HOSTPATH;
          pods[r].sys[(r / 5u) % 2u] = 3u;
          pods[r].ann[(r / 5u) % 2u] = uint2{3u, 0u};
        }
      }
      check_scatter(pods, T, "200 containers");
    }
  }
  {  // random tiles: every pod word field, lists of 0 to 5 items, three tiles and a partial one
    uint32_t s = 0xC0FFEEu;
    for (uint32_t round = 0; round < 50u; ++round) {
      std::vector<Pod> pods;
      const uint32_t n = 130u + rnd(s) % 90u;
      for (uint32_t r = 0; r < n; ++r) {
        Pod p;
        p.pw = rnd(s) & 0x7FFFFFu & ((rnd(s) & 3u) ? ~0u : 0u);
        for (uint32_t k = rnd(s) % 6u; k; --k) p.ctr.push_back(uint2{(rnd(s) & 1u) ? rnd(s) : 0u, rnd(s) & 0xFFFF07FFu});
        for (uint32_t k = rnd(s) % 6u; k; --k) {
          const uint32_t a = 1u << (rnd(s) % 29u), b = 1u << (rnd(s) % 29u);
          p.vol.push_back((rnd(s) % 5u) ? a : (rnd(s) & 1u) ? a | b : 0u);
        }
        for (uint32_t k = rnd(s) % 4u; k; --k) p.sys.push_back((rnd(s) & 7u) ? rnd(s) % 100u : KPE_NO_STR);
        for (uint32_t k = rnd(s) % 4u; k; --k) p.ann.push_back(uint2{rnd(s) % 50u, (rnd(s) & 3u) ? rnd(s) % 50u : KPE_NO_STR});
        pods.push_back(p);
      }
      check_scatter(pods, T, "random");
    }
  }
}

int main() {
  check_words();
  check_volumes();
  check_tiles();
  printf("lean_owner_check ok\n");
  return 0;
}
