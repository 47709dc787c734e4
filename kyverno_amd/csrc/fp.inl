// Row fingerprints (kpe_fetch_row_fingerprints, kpe_fingerprints_keep, kpe_changed_rows_fp): 8 bytes
// per row of an N x R verdict matrix, the sum over the row's cells with a response of a 64-bit hash
// of (the rule's salt, the verdict, the FAIL cell's check mask word). include/kpe.h states the rule.
// Included by results.hip (the body of kpe_row_fp_kernel) and by scripts/fp_check.cpp, which runs
// the same text lane by lane on the host under ASan / UBSan over buffers of exactly N x R bytes,
// N x R words and nrows x 8 bytes. The includer defines
//   KPE_FP_FN, KPE_FP_DEV      qualifiers of the arithmetic (the launcher and the host twin use it
//                              too) and of the phases
//   fp_load16(p, cnt, w)       cells [p, p + cnt) into w[4], cells past cnt zero; cnt <= 16 and p
//                              16-byte aligned (one 16-byte load when cnt == 16)
//   fp_lds_add(p, x)           *p += x on a 64-bit LDS word, atomically among the block's lanes
//
// A block takes groups of rpg whole rows (rpg * R <= kFpTile, or one row when a row is longer:
// R <= kFpMaxRules = kFpTile, so a row never is) and reads their contiguous bytes with aligned
// 16-byte loads: the group's first byte rounded down to 16, the cells before it skipped by index,
// the tail bounded by count. A lane sums its 16 cells in registers (with R >= 16 they lie in at most
// two rows: two registers, no row bookkeeping per cell) and adds each row's part to the row's LDS
// word. 64-bit integer adds commute: the result does not depend on the schedule.
constexpr uint32_t kFpTile = 4096;
constexpr uint32_t kFpMaxRules = 4096;  // a row fits the tile (KPE_DELTA_MAX_RULES)
constexpr uint32_t kFpMaxRows = 1024;   // rows of a group: 8 KiB of LDS words
constexpr uint32_t kFpLdsRules = 1024;  // both salt tables staged in LDS up to here (16 KiB), global past it
constexpr uint64_t kFpGold = 0x9E3779B97F4A7C15ull;
static_assert(kFpMaxRules <= kFpTile, "a row fits the tile");

// the splitmix64 finaliser: a bijection, mix64(0) == 0
KPE_FP_FN uint64_t fp_mix64(uint64_t z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
// One cell with a response (v != KPE_NA): tbl = [salts: R][msg_salts: R]; m = the cell's mask word,
// or 0 when it does not count.
KPE_FP_FN uint64_t fp_cell(uint32_t v, uint32_t m, const uint64_t* tbl, uint32_t col, uint32_t R, uint32_t msg_codes) {
  const bool msg = v < 8u && ((msg_codes >> v) & 1u);
  const uint64_t s = tbl[(msg ? R : 0u) + col];
  return fp_mix64(s + kFpGold * ((uint64_t)v | ((uint64_t)m << 8)));
}
KPE_FP_FN uint32_t fp_rows_per_group(uint32_t R) {
  const uint32_t r = kFpTile / (R ? R : 1u);
  return r < 1u ? 1u : (r > kFpMaxRows ? kFpMaxRows : r);
}
KPE_FP_FN uint32_t fp_byte(const uint32_t* w, uint32_t k) { return (w[k >> 2] >> (8u * (k & 3u))) & 0xFFu; }

// Group g of the window [row0, row0 + nrows): rows r0 .. r0 + rn relative to row0, the bytes
// [b0, b1) of the matrix and the aligned start a0 <= b0.
struct FpGroup {
  uint64_t r0;
  uint32_t rn;
  uint64_t b0, b1, a0;
};
KPE_FP_FN FpGroup fp_group(uint64_t g, uint64_t row0, uint64_t nrows, uint32_t R, uint32_t rpg) {
  FpGroup G;
  G.r0 = g * rpg;
  G.rn = nrows - G.r0 < rpg ? (uint32_t)(nrows - G.r0) : rpg;
  G.b0 = (row0 + G.r0) * R, G.b1 = G.b0 + (uint64_t)G.rn * R;
  G.a0 = G.b0 & ~(uint64_t)15u;
  return G;
}

// Phase 1 (lane t of 256): clear the group's row words.
KPE_FP_DEV void fp_clear(const FpGroup& G, uint32_t t, uint64_t* s_fp) {
  for (uint32_t i = t; i < G.rn; i += 256u) s_fp[i] = 0u;
}
// Phase 2: the cells. masks (MASKS only): N x R words, read for FAIL (2) cells alone. A word of four
// KPE_NA cells is passed over; so is every NA cell: no table read, no hash.
template <bool MASKS>
KPE_FP_DEV void fp_accum(const FpGroup& G, uint32_t t, const uint8_t* v, const uint32_t* masks, uint32_t R,
                         const uint64_t* tbl, uint32_t msg_codes, uint64_t* s_fp) {
  for (uint64_t c0 = G.a0 + t * 16u; c0 < G.b1; c0 += kFpTile) {
    const uint32_t cnt = G.b1 - c0 < 16u ? (uint32_t)(G.b1 - c0) : 16u;
    const uint32_t k0 = c0 < G.b0 ? (uint32_t)(G.b0 - c0) : 0u;  // c0 may start up to 15 cells before the group
    if (k0 >= cnt) continue;
    uint32_t w[4];
    fp_load16(v + c0, cnt, w);
    const uint32_t rel = (uint32_t)(c0 + k0 - G.b0);
    uint32_t lrow = rel / R, col = rel - lrow * R;
    if (R >= 16u) {  // uniform: cell k is in row lrow, or in lrow + 1 once its column wraps
      uint64_t acc0 = 0, acc1 = 0;
      // bit k: cell k holds a response and lies in the group. Most cells of a wide matrix are NA:
      // a lane walks its own set bits, so a wave hashes as often as its busiest lane has
      // responses, not 16 times.
      uint32_t nz = 0;
#pragma unroll
      for (uint32_t q = 0; q < 4u; ++q) {
        if (w[q] == 0u) continue;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j)
          if (fp_byte(w, 4u * q + j)) nz |= 1u << (4u * q + j);
      }
      nz &= (0xFFFFu << k0) & (0xFFFFu >> (16u - cnt));  // k0 <= k < cnt; 1 <= cnt <= 16
      const uint64_t lo = (uint64_t)w[0] | ((uint64_t)w[1] << 32), hi = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
      while (nz) {
        const uint32_t k = (uint32_t)__builtin_ctz(nz);
        nz &= nz - 1u;
        const uint32_t x = (uint32_t)((k < 8u ? lo >> (8u * k) : hi >> (8u * (k - 8u))) & 0xFFu);
        const uint32_t ck = col + (k - k0);  // < 2 R
        const bool next = ck >= R;
        uint32_t m = 0;
        if (MASKS && x == 2u) m = masks[c0 + k];
        const uint64_t h = fp_cell(x, m, tbl, next ? ck - R : ck, R, msg_codes);
        acc0 += next ? 0u : h;
        acc1 += next ? h : 0u;
      }
      if (acc0) fp_lds_add(&s_fp[lrow], acc0);
      if (acc1) fp_lds_add(&s_fp[lrow + 1u], acc1);  // non-zero only when a hashed cell lies in that row
    } else {
      uint64_t acc = 0;
#pragma unroll
      for (uint32_t k = 0; k < 16u; ++k) {
        if (k >= k0 && k < cnt) {
          const uint32_t x = fp_byte(w, k);
          if (x != 0u) {
            uint32_t m = 0;
            if (MASKS && x == 2u) m = masks[c0 + k];
            acc += fp_cell(x, m, tbl, col, R, msg_codes);
          }
          if (++col == R) {
            if (acc) fp_lds_add(&s_fp[lrow], acc);
            acc = 0, col = 0, ++lrow;
          }
        }
      }
      if (acc) fp_lds_add(&s_fp[lrow], acc);
    }
  }
}
// Phase 3: each row's 8 bytes, written once. out: the window's nrows words.
KPE_FP_DEV void fp_write(const FpGroup& G, uint32_t t, const uint64_t* s_fp, uint64_t* out) {
  for (uint32_t i = t; i < G.rn; i += 256u) out[G.r0 + i] = s_fp[i];
}
