// Host run of the bodies of kpe_report_need_count_kernel and kpe_report_need_scatter_kernel
// (kyverno_amd/csrc/report_rows.inl, the text the kernels run) under ASan / UBSan: the 256 lanes of
// each block in turn, phase by phase where the kernels have a barrier, over heap buffers of exactly
// nrows x R bytes (the compact matrix), N x R words (mask words), N x nmsg words (condition trace
// words), 3 R bytes and R words (the tables) and min(total, cap) entries per output array, so a read
// past a matrix, a misaligned 16-byte access or a write past a cap is a sanitizer report or a failed
// check here, before the kernels ever run on a device. What the kernels do between the phases (the
// wave and block prefix sums) is restated as a plain running sum in lane order.
//
//   report_rows_check <case> <lists-out>
// case: u64 N, u64 nrows, u32 R, u32 grid, u32 nmsg, u32 0, u64 caps[3], u8 need[3 R]
// ([mask][cond][pattern]), u32 slot[R] (KPE_RR_SLOT), u64 rows[nrows], u8 v[N R], u32 masks[N R],
// u32 mtrace[N nmsg]. Writes u64 totals[3], then mask_cells, mask_words, cond_cells, cond_words,
// pattern_cells, pattern_abs, each min(total, cap) entries; exits non-zero when they differ from the
// double loop over the listed rows (tests/test_report_rows_host.py compares them again in numpy).
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

#define CHECK(x)                                                          \
  do {                                                                    \
    if (!(x)) {                                                           \
      fprintf(stderr, "report_rows_check: %s (line %d)\n", #x, __LINE__); \
      exit(2);                                                            \
    }                                                                     \
  } while (0)

#define KPE_RR_FN static inline
#define KPE_RR_DEV static inline
static inline void rr_load16(const uint8_t* p, uint32_t cnt, uint32_t* w) {
  CHECK(((uintptr_t)p & 15u) == 0 && cnt >= 1 && cnt <= 16);
  w[0] = w[1] = w[2] = w[3] = 0;
  memcpy(w, p, cnt);  // the device reads 16 bytes only when cnt == 16
}
#include "../kyverno_amd/csrc/report_rows.inl"

constexpr uint32_t kLdsRules = 16384;  // results.hip kSelLdsRules: the tables are staged up to here

template <class T>
static T* exact(size_t n) {  // exactly n elements, 16-byte aligned like a device allocation
  const size_t bytes = n * sizeof(T);
  T* p = static_cast<T*>(malloc(bytes ? bytes : 1));
  CHECK(p && ((uintptr_t)p & 15u) == 0);
  return p;
}
template <class T>
static T* read_exact(FILE* f, size_t n) {
  T* p = exact<T>(n);
  CHECK(fread(p, sizeof(T), n, f) == n);
  return p;
}

int main(int argc, char** argv) {
  if (argc != 3) return fprintf(stderr, "usage: report_rows_check <case> <lists-out>\n"), 2;
  FILE* f = fopen(argv[1], "rb");
  CHECK(f);
  uint64_t nn[2], caps[3];
  uint32_t hdr[4];
  CHECK(fread(nn, 8, 2, f) == 2 && fread(hdr, 4, 4, f) == 4 && fread(caps, 8, 3, f) == 3);
  const uint64_t N = nn[0], nrows = nn[1];
  const uint32_t R = hdr[0], grid = hdr[1], nmsg = hdr[2];
  CHECK(R >= 1 && grid >= 1 && N >= 1);
  uint8_t* need_g = read_exact<uint8_t>(f, 3 * (size_t)R);
  uint32_t* slot = read_exact<uint32_t>(f, R);
  uint64_t* rows = read_exact<uint64_t>(f, nrows);
  uint8_t* v = read_exact<uint8_t>(f, N * R);
  uint32_t* masks = read_exact<uint32_t>(f, N * R);
  uint32_t* mtrace = read_exact<uint32_t>(f, N * nmsg);
  fclose(f);
  for (uint32_t r = 0; r < R; ++r) {  // what the caller of the kernels guarantees
    CHECK(!((need_g[r] | need_g[R + r] | need_g[2 * R + r]) & 1u));
    CHECK(KPE_RR_SLOT_WIDTH(slot[r]) ? KPE_RR_SLOT_FIRST(slot[r]) + KPE_RR_SLOT_WIDTH(slot[r]) <= nmsg : !need_g[R + r]);
  }
  for (uint64_t k = 0; k < nrows; ++k) CHECK(rows[k] < N);

  // the compact matrix (kpe_gather_rows_kernel's result)
  const uint64_t cells = nrows * R;
  uint8_t* cv = exact<uint8_t>(cells);
  for (uint64_t k = 0; k < nrows; ++k) memcpy(cv + k * R, v + rows[k] * R, R);
  const uint64_t ntiles = (cells + kRrTile - 1) / kRrTile;

  // a block's tables: staged copies of exactly 3 R bytes (one per block), or the global ones
  auto stage = [&]() -> uint8_t* {
    if (R > kLdsRules) return need_g;
    uint8_t* l = exact<uint8_t>(3 * (size_t)R);
    memcpy(l, need_g, 3 * (size_t)R);
    return l;
  };
  auto unstage = [&](uint8_t* l) {
    if (l != need_g) free(l);
  };

  // pass 1: three counts per tile
  uint32_t* counts = exact<uint32_t>(kRrKinds * ntiles);
  memset(counts, 0xEE, kRrKinds * ntiles * 4);
  for (uint32_t b = 0; b < grid && b < ntiles; ++b) {
    uint8_t* need = stage();
    for (uint64_t tile = b; tile < ntiles; tile += grid) {
      uint32_t sum[kRrKinds] = {0, 0, 0};
      for (uint32_t t = 0; t < 256; ++t) {
        uint32_t m[kRrKinds];
        rr_lane_hits(cv, cells, R, tile, t, need, m);
        for (uint32_t k = 0; k < kRrKinds; ++k) sum[k] += (uint32_t)__builtin_popcount(m[k]);
      }
      for (uint32_t k = 0; k < kRrKinds; ++k) {
        CHECK(counts[k * ntiles + tile] == 0xEEEEEEEEu);  // a tile's count is written once
        counts[k * ntiles + tile] = sum[k];
      }
    }
    unstage(need);
  }
  // pass 2: the exclusive scan of the 3 * ntiles counts (kpe_select_scan_kernel's result)
  uint64_t* offs = exact<uint64_t>(kRrKinds * ntiles + 1);
  offs[0] = 0;
  for (uint64_t i = 0; i < kRrKinds * ntiles; ++i) offs[i + 1] = offs[i] + counts[i];
  uint64_t total[kRrKinds], m_[kRrKinds];
  for (uint32_t k = 0; k < kRrKinds; ++k) {
    total[k] = offs[(k + 1) * ntiles] - offs[k * ntiles];
    m_[k] = total[k] < caps[k] ? total[k] : caps[k];
  }

  // pass 3: outputs of exactly min(total, cap) entries
  KpeRrSrc S{rows, masks, mtrace, slot, nmsg, 0u};
  KpeRrOut O{exact<uint64_t>(m_[0]), exact<uint32_t>(m_[0]),     m_[0], exact<uint64_t>(m_[1]), exact<uint32_t>(m_[1] * 4),
             m_[1],                  exact<uint64_t>(m_[2]),     exact<uint64_t>(m_[2]), m_[2]};
  memset(O.mask_cells, 0xDD, m_[0] * 8), memset(O.cond_cells, 0xDD, m_[1] * 8), memset(O.pattern_cells, 0xDD, m_[2] * 8);
  uint64_t live_tiles = 0;
  for (uint32_t b = 0; b < grid && b < ntiles; ++b) {
    uint8_t* need = stage();
    for (uint64_t tile = b; tile < ntiles; tile += grid) {
      uint64_t o0[kRrKinds], o1[kRrKinds];
      for (uint32_t k = 0; k < kRrKinds; ++k) {
        o0[k] = offs[k * ntiles + tile] - offs[k * ntiles];
        o1[k] = offs[k * ntiles + tile + 1] - offs[k * ntiles];
      }
      if (!rr_tile_live(o0, o1, O)) continue;
      ++live_tiles;
      uint64_t o[kRrKinds] = {o0[0], o0[1], o0[2]};  // tile offset + the lanes before, in lane order
      for (uint32_t t = 0; t < 256; ++t) {
        uint32_t m[kRrKinds];
        rr_lane_hits(cv, cells, R, tile, t, need, m);
        rr_lane_scatter(rr_lane_first(tile, t), m, o, R, S, O);
        for (uint32_t k = 0; k < kRrKinds; ++k) o[k] += (uint32_t)__builtin_popcount(m[k]);
      }
      for (uint32_t k = 0; k < kRrKinds; ++k) CHECK(o[k] == o1[k]);
    }
    unstage(need);
  }

  // the double loop over the listed rows
  uint64_t n[kRrKinds] = {0, 0, 0}, bad = 0;
  for (uint64_t k = 0; k < nrows; ++k)
    for (uint32_t r = 0; r < R; ++r) {
      const uint64_t cell = k * R + r, src = rows[k] * R + r;
      const uint32_t x = v[src];
      if (x >= 8u) continue;
      if ((need_g[r] >> x) & 1u) {
        if (n[0] < m_[0]) bad += O.mask_cells[n[0]] != cell || O.mask_words[n[0]] != masks[src];
        ++n[0];
      }
      if ((need_g[R + r] >> x) & 1u) {
        if (n[1] < m_[1]) {
          bad += O.cond_cells[n[1]] != cell;
          for (uint32_t q = 0; q < 4; ++q) {
            const uint32_t want =
                q < KPE_RR_SLOT_WIDTH(slot[r]) ? mtrace[rows[k] * nmsg + KPE_RR_SLOT_FIRST(slot[r]) + q] : 0u;
            bad += O.cond_words[n[1] * 4 + q] != want;
          }
        }
        ++n[1];
      }
      if ((need_g[2 * R + r] >> x) & 1u) {
        if (n[2] < m_[2]) bad += O.pattern_cells[n[2]] != cell || O.pattern_abs[n[2]] != src;
        ++n[2];
      }
    }
  for (uint32_t k = 0; k < kRrKinds; ++k) bad += n[k] != total[k];

  FILE* o = fopen(argv[2], "wb");
  CHECK(o && fwrite(total, 8, 3, o) == 3);
  CHECK(fwrite(O.mask_cells, 8, m_[0], o) == m_[0] && fwrite(O.mask_words, 4, m_[0], o) == m_[0]);
  CHECK(fwrite(O.cond_cells, 8, m_[1], o) == m_[1] && fwrite(O.cond_words, 16, m_[1], o) == m_[1]);
  CHECK(fwrite(O.pattern_cells, 8, m_[2], o) == m_[2] && fwrite(O.pattern_abs, 8, m_[2], o) == m_[2]);
  fclose(o);
  printf("N=%llu nrows=%llu R=%u tiles=%llu live=%llu totals=%llu/%llu/%llu written=%llu/%llu/%llu bad=%llu\n",
         (unsigned long long)N, (unsigned long long)nrows, R, (unsigned long long)ntiles, (unsigned long long)live_tiles,
         (unsigned long long)total[0], (unsigned long long)total[1], (unsigned long long)total[2],
         (unsigned long long)m_[0], (unsigned long long)m_[1], (unsigned long long)m_[2], (unsigned long long)bad);
  free(need_g), free(slot), free(rows), free(v), free(masks), free(mtrace), free(cv), free(counts), free(offs);
  free(O.mask_cells), free(O.mask_words), free(O.cond_cells), free(O.cond_words), free(O.pattern_cells), free(O.pattern_abs);
  return bad ? 1 : 0;
}
