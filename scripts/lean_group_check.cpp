// Host check (ASan / UBSan) of the group form of the LEAN evaluation's scatter (lean.inl
// l6_group_tiles) and of the quarter its item words carry, from the functions the kernels and the
// host themselves call (kyverno_amd/csrc/kernels_abi.h kpe_l6_tag_*):
//
//  (a) the builders and getters with a quarter: kpe_l6_tagq_id / kpe_l6_tagq_vol give words whose
//      owner, quarter, id (volume index, escape flag, decision) and slot (4 * owner + quarter:
//      byte 3) come back for all 4 quarters and 64 owners; the builders without a quarter
//      (kpe_l6_tag_id, kpe_l6_tag_vol, kpe_l6_tag_ctr's owner) give quarter 0 and the owners they
//      gave before; a masked KPE_NO_STR stays past every dictionary the columns are built for;
//  (b) a lane-by-lane model of the group scatter (per wave of four tiles: 256 interleaved words
//      cleared once, containers per tile into word 4 * owner + j, the three lists streamed from
//      hdr[tile0] to hdr[min(tile0 + 4, ntiles)] in 64-slot sets, KPE_L6G_*_SETS loaded up front
//      whether or not they hold an item of the group and the rest in a loop, a set wholly past the
//      count skipped, a slot ORed when its index is below the group's count) against the per-tile
//      model (lean_owner_check's: mask by the tile's count, OR into acc[owner]) over hand-built
//      corpora: every pod's evidence word equal, and every load inside the allocation.
//
//   lean_group_check        exits 0 when all hold, 2 with the first mismatch otherwise
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
      fprintf(stderr, "lean_group_check: %s (line %d): ", #x, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                                      \
      fprintf(stderr, "\n");                                             \
      exit(2);                                                           \
    }                                                                    \
  } while (0)

static uint32_t vol_code(uint32_t v) { return ((v >> VS_HOSTPATH) & 1u) | ((v & PSS_ALLOWED_VOLUMES) ? 0u : 2u); }

static void check_words() {
  static_assert(KPE_L6T_ID_MASK == 0xFFFFFFu, "ids are 24 bits under the quarter");
  const uint32_t sids[6] = {0u, 1u, 12345u, KPE_L6T_ID_MASK - 1u, KPE_L6T_ID_MASK, KPE_NO_STR};
  for (uint32_t owner = 0; owner < 64u; ++owner) {
    for (uint32_t id : sids) {
      const uint32_t w0 = kpe_l6_tag_id(id, owner);
      CHECK(kpe_l6_tag_owner(w0) == owner && kpe_l6_tag_quarter(w0) == 0u && kpe_l6_tag_get_id(w0) == (id & KPE_L6T_ID_MASK),
            "old id builder: id %#x owner %u word %#x", id, owner, w0);
      for (uint32_t q = 0; q < 4u; ++q) {
        const uint32_t w = kpe_l6_tagq_id(id, owner, q);
        CHECK(kpe_l6_tag_owner(w) == owner && kpe_l6_tag_quarter(w) == q && kpe_l6_tag_get_id(w) == (id & KPE_L6T_ID_MASK),
              "id %#x owner %u quarter %u word %#x", id, owner, q, w);
        CHECK(kpe_l6_tag_slot(w) == 4u * owner + q && kpe_l6_tag_slot(w) == (w >> 24), "slot: word %#x", w);
        CHECK((q ? w != w0 : w == w0), "quarter 0 is the old word: %#x %#x", w, w0);
      }
    }
    const uint32_t srcs[] = {0u, 1u << VS_HOSTPATH, 1u << VS_EMPTYDIR, 1u << VS_EPHEMERAL, (1u << VS_HOSTPATH) | (1u << VS_EMPTYDIR),
                             0x1FFFFFFFu};
    for (uint32_t m : srcs) {
      const uint32_t w0 = kpe_l6_tag_vol(m, owner);
      CHECK(kpe_l6_tag_owner(w0) == owner && kpe_l6_tag_quarter(w0) == 0u, "old volume builder: %#x owner %u word %#x", m, owner, w0);
      for (uint32_t q = 0; q < 4u; ++q) {
        const uint32_t w = kpe_l6_tagq_vol(m, owner, q);
        CHECK(kpe_l6_tag_owner(w) == owner && kpe_l6_tag_quarter(w) == q && kpe_l6_tag_slot(w) == 4u * owner + q,
              "volume %#x owner %u quarter %u word %#x", m, owner, q, w);
        CHECK((w & KPE_L6T_VOL_ESC) == (w0 & KPE_L6T_VOL_ESC) && (w & KPE_L6T_VOL_IDX) == (w0 & KPE_L6T_VOL_IDX),
              "the quarter touches the source: %#x %#x", w, w0);
        const bool multi = (m & (m - 1u)) != 0u;
        CHECK(multi == ((w & KPE_L6T_VOL_ESC) != 0u), "escape: sources %#x word %#x", m, w);
        if (!multi) CHECK(kpe_l6_vol_decide(w) == vol_code(m), "decision: sources %#x word %#x", m, w);
      }
    }
    const uint32_t wc = kpe_l6_tag_ctr(KPE_L6_CX_USED, 2047u, owner);  // the full word: owner only
    CHECK(kpe_l6_tag_owner(wc) == owner && kpe_l6_ctr_capset(wc) == 2047u, "container word %#x", wc);
  }
  CHECK(kpe_l6_tag_get_id(kpe_l6_tagq_id(KPE_NO_STR, 63u, 3u)) >= KPE_L6T_ID_MASK, "KPE_NO_STR masks to an id");
}

// ---- (b) the group scatter against the per-tile one ----
struct Pod {
  std::vector<uint2> ctr;     // {cx, cy}
  std::vector<uint32_t> vol;  // source masks
  std::vector<uint32_t> sys;  // ids
  std::vector<uint2> ann;     // {key id, value id}
};
static uint32_t cap_code(uint32_t id) { return (id * 5u + 3u) & 7u; }
static uint32_t sys_code(uint32_t id) { return id == (KPE_NO_STR & KPE_L6T_ID_MASK) ? 7u : (id * 3u) & 7u; }
static uint32_t ann_code(uint2 q) { return (q.x ^ (q.y >> 1)) & 3u; }

struct Columns {  // as kpe_lean_tag_kernel lays them out
  KpeL6TagLayout lay;
  std::vector<uint32_t> tag, vsrc, hdr;
  size_t n, ntiles;
  const char* what;
  uint32_t word(uint64_t byte) const {
    CHECK(byte + 4 <= lay.bytes, "%s: a load at byte %llu of %llu", what, (unsigned long long)byte, (unsigned long long)lay.bytes);
    return tag[byte / 4];
  }
};

static Columns build(const std::vector<Pod>& pods, const char* what) {
  Columns C;
  C.what = what, C.n = pods.size(), C.ntiles = (C.n + 63) / 64;
  size_t nctr = 0, nvol = 0, nsys = 0, nann = 0;
  for (const Pod& p : pods) nctr += p.ctr.size(), nvol += p.vol.size(), nsys += p.sys.size(), nann += p.ann.size();
  C.lay = kpe_l6_tag_layout((uint32_t)nctr, (uint32_t)nvol, (uint32_t)nsys, (uint32_t)nann);
  C.tag.assign(C.lay.bytes / 4, 0u);
  C.hdr.assign(4 * (C.ntiles + 1), 0u);
  size_t c = 0, v = 0, s = 0, a = 0;
  for (size_t r = 0; r < C.n; ++r) {
    uint32_t* h = &C.hdr[4 * (r >> 6)];
    if (!(r & 63)) h[0] = (uint32_t)c, h[1] = (uint32_t)v, h[2] = (uint32_t)s, h[3] = (uint32_t)a;
    const uint32_t o = (uint32_t)(r & 63), q = (uint32_t)((r >> 6) & 3);
    for (const uint2& e : pods[r].ctr) C.tag[c++] = kpe_l6_tag_ctr(e.x, e.y, o);
    for (uint32_t m : pods[r].vol) C.tag[C.lay.o_vol / 4 + v++] = kpe_l6_tagq_vol(m, o, q), C.vsrc.push_back(m);
    for (uint32_t id : pods[r].sys) C.tag[C.lay.o_sys / 4 + s++] = kpe_l6_tagq_id(id, o, q);
    for (const uint2& k : pods[r].ann)
      C.tag[C.lay.o_ann / 4 + 2 * a] = kpe_l6_tagq_id(k.x, o, q), C.tag[C.lay.o_ann / 4 + 2 * a + 1] = k.y, ++a;
  }
  uint32_t* h = &C.hdr[4 * C.ntiles];
  h[0] = (uint32_t)c, h[1] = (uint32_t)v, h[2] = (uint32_t)s, h[3] = (uint32_t)a;
  return C;
}

static uint32_t ctr_ev(uint32_t e) { return (e & ((1u << KPE_L6C_STATES) - 1u)) | (cap_code(kpe_l6_ctr_capset(e)) << KPE_L6C_CAP_SH); }

// the per-tile model: every row's evidence word (lean_owner_check's check_scatter)
static std::vector<uint32_t> per_tile(const Columns& C) {
  std::vector<uint32_t> out(C.ntiles * 64, 0u);
  auto slots = [](uint32_t first, uint32_t count) { return count <= first ? first : first + ((count - first + 63u) / 64u) * 64u; };
  for (size_t t = 0; t < C.ntiles; ++t) {
    const uint32_t* h = &C.hdr[4 * t];
    const uint32_t nct = h[4] - h[0], nvt = h[5] - h[1], nst = h[6] - h[2], nat = h[7] - h[3];
    uint32_t* acc = &out[64 * t];
    for (uint32_t s = 0; s < slots(KPE_L6_CTR, nct); ++s) {
      const uint32_t e = C.word(4ull * (h[0] + s));
      acc[kpe_l6_tag_owner(e)] |= s < nct ? ctr_ev(e) : 0u;
    }
    for (uint32_t s = 0; s < slots(KPE_L6_VOL, nvt); ++s) {
      const uint32_t w = C.word(C.lay.o_vol + 4ull * (h[1] + s));
      uint32_t c = kpe_l6_vol_decide(w);
      if (s < nvt && (w & KPE_L6T_VOL_ESC)) c = vol_code(C.vsrc[h[1] + s]);
      acc[kpe_l6_tag_owner(w)] |= s < nvt ? c << KPE_L6C_VOL_SH : 0u;
    }
    for (uint32_t s = 0; s < slots(KPE_L6_SMALL, nst); ++s) {
      const uint32_t w = C.word(C.lay.o_sys + 4ull * (h[2] + s));
      acc[kpe_l6_tag_owner(w)] |= s < nst ? sys_code(kpe_l6_tag_get_id(w)) << KPE_L6C_SYS_SH : 0u;
    }
    for (uint32_t s = 0; s < slots(KPE_L6_SMALL, nat); ++s) {
      const uint32_t k = C.word(C.lay.o_ann + 8ull * (h[3] + s)), v = C.word(C.lay.o_ann + 8ull * (h[3] + s) + 4);
      acc[kpe_l6_tag_owner(k)] |= s < nat ? ann_code(uint2{kpe_l6_tag_get_id(k), v}) << KPE_L6C_ANN_SH : 0u;
    }
  }
  return out;
}

// the group model, lane by lane as l6_group_tiles runs: one wave per four tiles
static std::vector<uint32_t> per_group(const Columns& C) {
  std::vector<uint32_t> out(C.ntiles * 64, 0u);
  const uint32_t nt = (uint32_t)C.ntiles;
  for (uint32_t tile0 = 0; tile0 < nt; tile0 += 4u) {
    // lane k's header word: word k & 3 of hdr[min(tile0 + k / 4, ntiles)]
    uint32_t hall[20];
    for (uint32_t k = 0; k < 20u; ++k) hall[k] = C.hdr[4 * (tile0 + (k >> 2) < nt ? tile0 + (k >> 2) : nt) + (k & 3u)];
    uint32_t acc[256];
    memset(acc, 0, sizeof acc);
    auto put = [&](uint32_t w, uint32_t ev, bool valid) {
      const uint32_t i = kpe_l6_tag_slot(w);
      CHECK(i < 256u, "%s: word index %u", C.what, i);
      acc[i] |= valid ? ev : 0u;
    };
    for (uint32_t j = 0; j < 4u && tile0 + j < nt; ++j) {
      const uint32_t C0 = hall[4 * j], nct = hall[4 * j + 4] - C0;
      for (uint32_t b = 0; b < KPE_L6_CTR || b < nct; b += 64u)  // two sets loaded whatever they hold, then the loop
        for (uint32_t lane = 0; lane < 64u; ++lane) {
          const uint32_t e = C.word(4ull * (C0 + b + lane));
          acc[4u * kpe_l6_tag_owner(e) + j] |= b + lane < nct ? ctr_ev(e) : 0u;
        }
    }
    const uint32_t V0 = hall[1], S0 = hall[2], A0 = hall[3];
    const uint32_t nvg = hall[17] - V0, nsg = hall[18] - S0, nag = hall[19] - A0;
    // the sets loaded up front are loaded whether or not the group has that many items
    for (uint32_t s = 0; s < KPE_L6G_VOL_SETS; ++s)
      for (uint32_t lane = 0; lane < 64u; ++lane) (void)C.word(C.lay.o_vol + 4ull * (V0 + 64u * s + lane));
    for (uint32_t s = 0; s < KPE_L6G_SYS_SETS; ++s)
      for (uint32_t lane = 0; lane < 64u; ++lane) (void)C.word(C.lay.o_sys + 4ull * (S0 + 64u * s + lane));
    for (uint32_t s = 0; s < KPE_L6G_ANN_SETS; ++s)
      for (uint32_t lane = 0; lane < 64u; ++lane) (void)C.word(C.lay.o_ann + 8ull * (A0 + 64u * s + lane) + 4);
    for (uint32_t b = 0; b < nvg; b += 64u)  // a set wholly past the count is skipped
      for (uint32_t lane = 0; lane < 64u; ++lane) {
        const uint32_t w = C.word(C.lay.o_vol + 4ull * (V0 + b + lane));
        uint32_t c = kpe_l6_vol_decide(w);
        if (b + lane < nvg && (w & KPE_L6T_VOL_ESC)) c = vol_code(C.vsrc[V0 + b + lane]);
        put(w, c << KPE_L6C_VOL_SH, b + lane < nvg);
      }
    for (uint32_t b = 0; b < nsg; b += 64u)
      for (uint32_t lane = 0; lane < 64u; ++lane) {
        const uint32_t w = C.word(C.lay.o_sys + 4ull * (S0 + b + lane));
        put(w, sys_code(kpe_l6_tag_get_id(w)) << KPE_L6C_SYS_SH, b + lane < nsg);
      }
    for (uint32_t b = 0; b < nag; b += 64u)
      for (uint32_t lane = 0; lane < 64u; ++lane) {
        const uint32_t k = C.word(C.lay.o_ann + 8ull * (A0 + b + lane)), v = C.word(C.lay.o_ann + 8ull * (A0 + b + lane) + 4);
        put(k, ann_code(uint2{kpe_l6_tag_get_id(k), v}) << KPE_L6C_ANN_SH, b + lane < nag);
      }
    // lane i reads words 4 i .. 4 i + 3: its pod of each tile
    for (uint32_t j = 0; j < 4u && tile0 + j < nt; ++j)
      for (uint32_t lane = 0; lane < 64u; ++lane) out[64 * (tile0 + j) + lane] = acc[4u * lane + j];
  }
  return out;
}

// the evidence word straight from the pod's own items
static uint32_t direct(const Pod& p) {
  uint32_t ev = 0;
  for (const uint2& e : p.ctr) ev |= ctr_ev(kpe_l6_tag_ctr(e.x, e.y, 0u));
  for (uint32_t m : p.vol) ev |= vol_code(m) << KPE_L6C_VOL_SH;
  for (uint32_t id : p.sys) ev |= sys_code(id & KPE_L6T_ID_MASK) << KPE_L6C_SYS_SH;
  for (const uint2& q : p.ann) ev |= ann_code(uint2{q.x & KPE_L6T_ID_MASK, q.y}) << KPE_L6C_ANN_SH;
  return ev;
}

static void compare(const std::vector<Pod>& pods, const char* what) {
  const Columns C = build(pods, what);
  const std::vector<uint32_t> a = per_tile(C), b = per_group(C);
  for (size_t r = 0; r < pods.size(); ++r) {
    CHECK(a[r] == b[r], "%s: row %zu per tile %#x, group %#x", what, r, a[r], b[r]);
    CHECK(b[r] == direct(pods[r]), "%s: row %zu group %#x, its own items %#x", what, r, b[r], direct(pods[r]));
  }
}

static Pod clean_pod() { return Pod{{uint2{0u, 1u}}, {1u << VS_EMPTYDIR}, {}, {}}; }
static Pod bad_pod(uint32_t r) {
  Pod p;
  p.ctr = {uint2{CX_PRIV_T, 2047u}, uint2{KPE_L6_CX_USED, 7u}};
  p.vol = {1u << VS_HOSTPATH, (1u << VS_HOSTPATH) | (1u << VS_EMPTYDIR), 0u};
  p.sys = {5u + r, KPE_NO_STR};
  p.ann = {uint2{1u, 0u}, uint2{2u, KPE_NO_STR}};
  return p;
}
static uint32_t rnd(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

static void check_groups() {
  {  // a clean group of four tiles with few items, its last tile followed at once by the next
    // group's offending items in every list: the slots past the first group's counts hold them,
    // and their owners 0, 1, 2, ... and quarter 0 name the first group's pods
    std::vector<Pod> pods;
    for (uint32_t r = 0; r < 256u; ++r) {
      Pod p = clean_pod();
      if (r % 3u == 0u) p.ctr.clear(), p.vol.clear();
      if (r % 7u == 1u) p.sys = {0u}, p.ann = {uint2{0u, 0u}};
      pods.push_back(p);
    }
    for (uint32_t r = 0; r < 256u; ++r) pods.push_back(r < 40u || r % 64u < 3u ? bad_pod(r) : clean_pod());
    compare(pods, "clean group then offending group");
  }
  for (uint32_t n : {1u, 63u, 64u, 65u, 129u, 192u, 193u, 256u + 1u, 256u + 130u}) {
    // a last group of fewer than four tiles (and a partial last tile), offenders at both ends
    std::vector<Pod> pods;
    for (uint32_t r = 0; r < n; ++r) pods.push_back(r % 9u == 0u || r + 1u == n ? bad_pod(r) : clean_pod());
    compare(pods, "short last group");
  }
  {  // tiles with no item of a list: volumes only in tile 1, sysctls only in tile 3, annotations
    // only in tile 0, no containers in tile 2; and a whole group with no item at all before them
    std::vector<Pod> pods(256);
    for (uint32_t r = 0; r < 256u; ++r) {
      Pod p;
      const uint32_t t = r >> 6;
      if (t != 2u) p.ctr = {uint2{r % 5u ? 0u : CX_HOSTPORT, 3u}};
      if (t == 1u) p.vol = {r % 4u ? 1u << VS_SECRET : 1u << VS_NFS};
      if (t == 3u) p.sys = {r % 6u};
      if (t == 0u) p.ann = {uint2{r % 4u, r % 3u}};
      pods.push_back(p);
    }
    compare(pods, "tiles with empty lists");
  }
  {  // more items than the sets loaded up front: one pod with 500 volumes, one with 200 sysctls,
    // one with 300 annotations and one with 200 containers, the offender at each position in turn
    for (uint32_t at : {0u, 63u, 64u, 127u, 128u, 199u}) {
      std::vector<Pod> pods;
      for (uint32_t r = 0; r < 300u; ++r) pods.push_back(clean_pod());
      pods[70].vol.assign(500, 1u << VS_SECRET), pods[70].vol[at + 300u] = 1u << VS_HOSTPATH;
      pods[70].vol[at] = (1u << VS_SECRET) | (1u << VS_GCEPD);  // several sources: the escape
      pods[130].sys.assign(200, 0u), pods[130].sys[at] = 3u;
      pods[200].ann.assign(300, uint2{0u, 0u}), pods[200].ann[at + 100u] = uint2{3u, 0u};
      pods[9].ctr.assign(200, uint2{0u, 1u}), pods[9].ctr[at] = uint2{CX_PRIV_T, 3u};
      pods[299] = bad_pod(0u);
      compare(pods, "more items than the sets loaded up front");
    }
    // exactly the up-front sets, and one more
    for (uint32_t extra : {0u, 1u}) {
      std::vector<Pod> pods;
      for (uint32_t r = 0; r < 512u; ++r) pods.push_back(Pod{});
      pods[5].vol.assign(64u * KPE_L6G_VOL_SETS + extra, 1u << VS_SECRET), pods[5].vol.back() = 1u << VS_HOSTPATH;
      pods[6].sys.assign(64u * KPE_L6G_SYS_SETS + extra, 0u), pods[6].sys.back() = 3u;
      pods[7].ann.assign(64u * KPE_L6G_ANN_SETS + extra, uint2{0u, 0u}), pods[7].ann.back() = uint2{3u, 0u};
      pods[256] = bad_pod(1u);
      compare(pods, "the up-front sets exactly, and one item more");
    }
  }
  {  // random groups: lists of 0 to 5 items, a few long ones
    uint32_t s = 0xC0FFEEu;
    for (uint32_t round = 0; round < 40u; ++round) {
      std::vector<Pod> pods;
      const uint32_t n = 200u + rnd(s) % 700u;
      for (uint32_t r = 0; r < n; ++r) {
        Pod p;
        const uint32_t big = rnd(s) % 97u == 0u ? 150u : 0u;
        for (uint32_t k = rnd(s) % 6u; k; --k) p.ctr.push_back(uint2{(rnd(s) & 1u) ? rnd(s) : 0u, rnd(s) & 0xFFFF07FFu});
        for (uint32_t k = rnd(s) % 6u + big; k; --k) {
          const uint32_t a = 1u << (rnd(s) % 29u), b = 1u << (rnd(s) % 29u);
          p.vol.push_back((rnd(s) % 5u) ? a : (rnd(s) & 1u) ? a | b : 0u);
        }
        for (uint32_t k = rnd(s) % 4u + (big & (rnd(s) & 1u ? ~0u : 0u)); k; --k) p.sys.push_back((rnd(s) & 7u) ? rnd(s) % 100u : KPE_NO_STR);
        for (uint32_t k = rnd(s) % 4u; k; --k) p.ann.push_back(uint2{rnd(s) % 50u, (rnd(s) & 3u) ? rnd(s) % 50u : KPE_NO_STR});
        pods.push_back(p);
      }
      compare(pods, "random");
    }
  }
}

int main() {
  check_words();
  check_groups();
  printf("lean_group_check ok\n");
  return 0;
}
