// The flag pass of kpe_changed_rows: which rows of a new N x Rn verdict matrix differ from a kept
// N x Ro one. Included by results.hip (the body of kpe_delta_flags_kernel) and by
// scripts/delta_check.cpp, which runs the same text lane by lane on the host under
// ASan / UBSan over buffers of exactly N x Ro and N x Rn bytes. The includer defines
//   KPE_DELTA_FN, KPE_DELTA_DEV         qualifiers of the index arithmetic (the launcher calls it on the
//                                       host too) and of the phases
//   delta_load16(p, cnt, w)             cells [p, p + cnt) into w[4], cells past cnt zero; cnt <= 16
//                                       and p 16-byte aligned (one 16-byte load when cnt == 16)
//   delta_store16(p, w)                 w[4] to 16-byte aligned LDS
//
// A block takes groups of rpg whole rows. Both sides of a group are at most kDeltaTile bytes
// (rpg * max(Rn, Ro) <= kDeltaTile, or one row when a row is longer: Rn, Ro <= kDeltaMaxRules =
// kDeltaTile, so a row never is). The kept rows are staged in LDS by aligned 16-byte loads: the
// group's first byte rounded down to 16, the skew removed by index. The new rows are read the same
// way and never staged; their skew is their own (Rn != Ro).
//
// LDS (dynamic, every carve a multiple of 16): [kept rows: old_bytes][row flags: rpg words]
// [tab: Rn words][unmapped: Ro bytes].
constexpr uint32_t kDeltaTile = 4096;
constexpr uint32_t kDeltaMaxRules = 4096;  // the most rules on either side: a row fits the tile,
                                           // a kept column fits tab's 16 bits, LDS <= 29 KiB
constexpr uint32_t kDeltaMaxRows = 1024;   // rows of a group
constexpr uint32_t kDeltaNone = 0xFFFFu;   // tab: no kept column
static_assert(kDeltaMaxRules <= kDeltaTile && kDeltaMaxRules < kDeltaNone, "a row fits the tile and tab");

KPE_DELTA_FN uint32_t delta_rows_per_group(uint32_t Rn, uint32_t Ro) {
  const uint32_t w = Rn > Ro ? Rn : Ro;
  const uint32_t r = kDeltaTile / (w ? w : 1u);
  return r < 1u ? 1u : (r > kDeltaMaxRows ? kDeltaMaxRows : r);
}
KPE_DELTA_FN uint32_t delta_up16(uint32_t x) { return (x + 15u) & ~15u; }
// LDS carve
struct DeltaLds {
  uint32_t old_bytes, flag_off, tab_off, unm_off, total;
};
KPE_DELTA_FN DeltaLds delta_lds(uint32_t Rn, uint32_t Ro, uint32_t rpg) {
  DeltaLds L;
  L.old_bytes = delta_up16(rpg * Ro + 15u);  // the skew (<= 15) + the rows, in whole 16-byte stores
  L.flag_off = L.old_bytes;
  L.tab_off = L.flag_off + delta_up16(rpg * 4u);
  L.unm_off = L.tab_off + delta_up16(Rn * 4u);
  L.total = L.unm_off + delta_up16(Ro);
  return L;
}

// Group g: rows [r0, r0 + rn); per side the group's bytes [b0, b1), the aligned start a0 <= b0 and
// the skew b0 - a0 (kept side: the LDS offset of the group's first cell).
struct DeltaGroup {
  uint64_t r0;
  uint32_t rn;
  uint64_t ob0, ob1, oa0, nb0, nb1, na0;
  uint32_t oskew;
};
KPE_DELTA_FN DeltaGroup delta_group(uint64_t g, uint64_t n, uint32_t Rn, uint32_t Ro, uint32_t rpg) {
  DeltaGroup G;
  G.r0 = g * rpg;
  G.rn = n - G.r0 < rpg ? (uint32_t)(n - G.r0) : rpg;
  G.ob0 = G.r0 * Ro, G.ob1 = G.ob0 + (uint64_t)G.rn * Ro;
  G.nb0 = G.r0 * Rn, G.nb1 = G.nb0 + (uint64_t)G.rn * Rn;
  G.oa0 = G.ob0 & ~(uint64_t)15u, G.na0 = G.nb0 & ~(uint64_t)15u;
  G.oskew = (uint32_t)(G.ob0 - G.oa0);
  return G;
}
KPE_DELTA_FN uint32_t delta_byte(const uint32_t* w, uint32_t k) { return (w[k >> 2] >> (8u * (k & 3u))) & 0xFFu; }

// Phase 1 (lane t of 256): clear the group's row flags, stage its kept rows. Nothing past the
// group's last byte, so nothing past N x Ro, is read.
KPE_DELTA_DEV void delta_stage(const DeltaGroup& G, uint32_t t, const uint8_t* vold, uint8_t* s_old, uint32_t* s_flag) {
  for (uint32_t i = t; i < G.rn; i += 256u) s_flag[i] = 0u;
  for (uint64_t c0 = G.oa0 + t * 16u; c0 < G.ob1; c0 += kDeltaTile) {
    const uint32_t cnt = G.ob1 - c0 < 16u ? (uint32_t)(G.ob1 - c0) : 16u;
    uint32_t w[4];
    delta_load16(vold + c0, cnt, w);
    delta_store16(s_old + (uint32_t)(c0 - G.oa0), w);
  }
}
// Phase 2a: the new cells against their partners. tab[col]: the kept column (bits 0-15,
// kDeltaNone: none, the partner is KPE_NA) and the column's `always` mask (bits 16-23). All
// writers of a row flag store 1.
KPE_DELTA_DEV void delta_compare(const DeltaGroup& G, uint32_t t, const uint8_t* vnew, uint32_t Rn, uint32_t Ro,
                                const uint32_t* s_tab, const uint8_t* s_old, uint32_t* s_flag) {
  for (uint64_t c0 = G.na0 + t * 16u; c0 < G.nb1; c0 += kDeltaTile) {
    const uint32_t cnt = G.nb1 - c0 < 16u ? (uint32_t)(G.nb1 - c0) : 16u;
    const uint32_t k0 = c0 < G.nb0 ? (uint32_t)(G.nb0 - c0) : 0u;  // c0 may start up to 15 cells before the group
    if (k0 >= cnt) continue;
    uint32_t w[4];
    delta_load16(vnew + c0, cnt, w);
    const uint32_t rel = (uint32_t)(c0 + k0 - G.nb0);
    uint32_t lrow = rel / Rn, col = rel - lrow * Rn;
    uint32_t obase = G.oskew + lrow * Ro;  // LDS offset of the kept row
#pragma unroll
    for (uint32_t k = 0; k < 16u; ++k) {
      if (k >= k0 && k < cnt) {
        const uint32_t x = delta_byte(w, k);
        const uint32_t e = s_tab[col];
        const uint32_t m = e & 0xFFFFu;
        const uint32_t o = m != kDeltaNone ? (uint32_t)s_old[obase + m] : 0u;
        if (x != o || (x < 8u && ((e >> (16u + x)) & 1u))) s_flag[lrow] = 1u;
        if (++col == Rn) col = 0u, ++lrow, obase += Ro;
      }
    }
  }
}
// Phase 2b (only when some kept column is unmapped): a response in such a column.
KPE_DELTA_DEV void delta_sweep(const DeltaGroup& G, uint32_t t, uint32_t Ro, const uint8_t* s_unm, const uint8_t* s_old,
                              uint32_t* s_flag) {
  const uint32_t nb = G.rn * Ro;
  for (uint32_t i = t; i < nb; i += 256u) {
    if (s_old[G.oskew + i] == 0u) continue;
    const uint32_t lrow = i / Ro;
    if (s_unm[i - lrow * Ro]) s_flag[lrow] = 1u;
  }
}
// Phase 3: each row's byte, written once.
KPE_DELTA_DEV void delta_write(const DeltaGroup& G, uint32_t t, const uint32_t* s_flag, uint8_t* flags) {
  for (uint32_t i = t; i < G.rn; i += 256u) flags[G.r0 + i] = s_flag[i] ? 1u : 0u;
}
