// The pass of kpe_results_splice: the new kept matrix K' (N x rn) from the kept one K (N x Ro) and the
// evaluation E (N x Rs) of the edited policies alone, with one flag byte per row. Included by
// results.hip (the body of kpe_splice_kernel) and by scripts/splice_check.cpp, which runs the same
// text lane by lane on the host under ASan / UBSan over buffers of exactly N x Ro, N x Rs, N x rn and
// N bytes. The includer defines
//   KPE_SPLICE_FN, KPE_SPLICE_DEV       qualifiers of the index arithmetic (the launcher calls it on
//                                       the host too) and of the phases
//   splice_load16(p, cnt, w)            global cells [p, p + cnt) into w[4], cells past cnt zero;
//                                       cnt <= 16 and p 16-byte aligned (one 16-byte load when cnt == 16)
//   splice_store16(p, w)                w[4] to 16-byte aligned global memory
//   splice_lds_store16(p, w), splice_lds_load16(p, w)   the same to / from 16-byte aligned LDS
//
// A block takes groups of rpg whole rows; each of a group's three sides is at most kSpliceTile bytes
// (rpg * max(Ro, Rs, rn) <= kSpliceTile; Ro, Rs, rn <= kSpliceMaxRules = kSpliceTile, so a row always
// fits). K and E rows are staged in LDS by aligned 16-byte loads: the group's first byte rounded
// down to 16, the skew removed by index, the tail bounded by count. K' rows are built in LDS with
// the skew of their place in the output, so the interior of the group leaves in aligned 16-byte
// stores and only the two ragged edges, whose 16-byte lines the neighbouring groups share, in byte
// stores.
//
// col: two words per output column. Word 0: the source column (bits 0-15) and kSpliceFromSub when
// it is a column of E, else of K. Word 1 (E columns only): the partner, the kept column of the same
// name (bits 0-15, kSpliceNone: none, the partner cell is KPE_NA), and the column's `always` mask
// (bits 16-23). Thirteen bits of source, thirteen of partner and eight of mask do not fit one word.
//
// LDS (dynamic, every carve a multiple of 16): [K rows][E rows][K' rows][row flags: rpg words]
// [col: 2 rn words][unmapped: Ro bytes].
constexpr uint32_t kSpliceTile = 4096;
constexpr uint32_t kSpliceMaxRules = 4096;  // KPE_DELTA_MAX_RULES: a row fits the tile, LDS <= 49 KiB
constexpr uint32_t kSpliceMaxRows = 1024;   // rows of a group
constexpr uint32_t kSpliceNone = 0xFFFFu;
constexpr uint32_t kSpliceFromSub = 0x80000000u;
static_assert(kSpliceMaxRules <= kSpliceTile && kSpliceMaxRules < kSpliceNone, "a row fits the tile and col");

KPE_SPLICE_FN uint32_t splice_rows_per_group(uint32_t Ro, uint32_t Rs, uint32_t rn) {
  uint32_t w = Ro > Rs ? Ro : Rs;
  w = w > rn ? w : rn;
  const uint32_t r = kSpliceTile / (w ? w : 1u);
  return r < 1u ? 1u : (r > kSpliceMaxRows ? kSpliceMaxRows : r);
}
KPE_SPLICE_FN uint32_t splice_up16(uint32_t x) { return (x + 15u) & ~15u; }
struct SpliceLds {
  uint32_t k_bytes, e_off, e_bytes, o_off, o_bytes, flag_off, col_off, unm_off, total;
};
KPE_SPLICE_FN SpliceLds splice_lds(uint32_t Ro, uint32_t Rs, uint32_t rn, uint32_t rpg) {
  SpliceLds L;
  L.k_bytes = splice_up16(rpg * Ro + 15u);  // the skew (<= 15) + the rows, in whole 16-byte stores
  L.e_off = L.k_bytes;
  L.e_bytes = splice_up16(rpg * Rs + 15u);
  L.o_off = L.e_off + L.e_bytes;
  L.o_bytes = splice_up16(rpg * rn + 15u);
  L.flag_off = L.o_off + L.o_bytes;
  L.col_off = L.flag_off + splice_up16(rpg * 4u);
  L.unm_off = L.col_off + splice_up16(rn * 8u);
  L.total = L.unm_off + splice_up16(Ro);
  return L;
}

// One side of a group: its bytes [b0, b1), the aligned start a0 <= b0, the skew b0 - a0 (the LDS
// offset of the group's first cell).
struct SpliceSide {
  uint64_t b0, b1, a0;
  uint32_t skew;
};
// Group g: rows [r0, r0 + rows).
struct SpliceGroup {
  uint64_t r0;
  uint32_t rows;
  SpliceSide k, e, o;
};
KPE_SPLICE_FN SpliceSide splice_side(uint64_t r0, uint32_t rows, uint32_t R) {
  SpliceSide S;
  S.b0 = r0 * R, S.b1 = S.b0 + (uint64_t)rows * R;
  S.a0 = S.b0 & ~(uint64_t)15u;
  S.skew = (uint32_t)(S.b0 - S.a0);
  return S;
}
KPE_SPLICE_FN SpliceGroup splice_group(uint64_t g, uint64_t n, uint32_t Ro, uint32_t Rs, uint32_t rn, uint32_t rpg) {
  SpliceGroup G;
  G.r0 = g * rpg;
  G.rows = n - G.r0 < rpg ? (uint32_t)(n - G.r0) : rpg;
  G.k = splice_side(G.r0, G.rows, Ro);
  G.e = splice_side(G.r0, G.rows, Rs);
  G.o = splice_side(G.r0, G.rows, rn);
  return G;
}

// Phase 1 (lane t of 256): clear the group's row flags, stage its K and E rows. Nothing past a
// side's last byte, so nothing past N x Ro or N x Rs, is read.
KPE_SPLICE_DEV void splice_stage_side(const SpliceSide& S, uint32_t t, const uint8_t* v, uint8_t* s_v) {
  for (uint64_t c0 = S.a0 + t * 16u; c0 < S.b1; c0 += 256u * 16u) {
    const uint32_t cnt = S.b1 - c0 < 16u ? (uint32_t)(S.b1 - c0) : 16u;
    uint32_t w[4];
    splice_load16(v + c0, cnt, w);
    splice_lds_store16(s_v + (uint32_t)(c0 - S.a0), w);
  }
}
KPE_SPLICE_DEV void splice_stage(const SpliceGroup& G, uint32_t t, const uint8_t* kept, const uint8_t* sub, uint8_t* s_k,
                                 uint8_t* s_e, uint32_t* s_flag) {
  for (uint32_t i = t; i < G.rows; i += 256u) s_flag[i] = 0u;
  splice_stage_side(G.k, t, kept, s_k);
  splice_stage_side(G.e, t, sub, s_e);
}
// Phase 2a: the K' rows, a word of four cells per lane and step, at their output skew. A cell of
// E is compared with its partner on the way; all writers of a row flag store 1. Cells of the
// first word before the group and of the last word past it are written as zero and never leave.
KPE_SPLICE_DEV void splice_build(const SpliceGroup& G, uint32_t t, uint32_t Ro, uint32_t Rs, uint32_t rn,
                                 const uint32_t* s_col, const uint8_t* s_k, const uint8_t* s_e, uint8_t* s_o,
                                 uint32_t* s_flag) {
  const uint32_t nb = G.rows * rn, skew = G.o.skew, end = skew + nb;
  for (uint32_t p = t * 4u; p < end; p += 256u * 4u) {
    uint32_t word = 0u;
    if (p + 4u > skew) {
      const uint32_t first = p < skew ? 0u : p - skew;
      uint32_t lrow = first / rn, col = first - lrow * rn;
#pragma unroll
      for (uint32_t k = 0; k < 4u; ++k) {
        if (p + k >= skew && p + k < end) {
          const uint32_t src = s_col[2u * col];
          uint32_t x;
          if (src & kSpliceFromSub) {
            x = s_e[G.e.skew + lrow * Rs + (src & 0xFFFFu)];
            const uint32_t e = s_col[2u * col + 1u];
            const uint32_t m = e & 0xFFFFu;
            const uint32_t o = m != kSpliceNone ? (uint32_t)s_k[G.k.skew + lrow * Ro + m] : 0u;
            if (x != o || (x < 8u && ((e >> (16u + x)) & 1u))) s_flag[lrow] = 1u;
          } else {
            x = s_k[G.k.skew + lrow * Ro + src];
          }
          word |= x << (8u * k);
          if (++col == rn) col = 0u, ++lrow;
        }
      }
    }
    *reinterpret_cast<uint32_t*>(s_o + p) = word;
  }
}
// Phase 2b (only when some kept column is neither copied nor a partner): a response in such a column.
KPE_SPLICE_DEV void splice_sweep(const SpliceGroup& G, uint32_t t, uint32_t Ro, const uint8_t* s_unm, const uint8_t* s_k,
                                 uint32_t* s_flag) {
  const uint32_t nb = G.rows * Ro;
  for (uint32_t i = t; i < nb; i += 256u) {
    if (s_k[G.k.skew + i] == 0u) continue;
    const uint32_t lrow = i / Ro;
    if (s_unm[i - lrow * Ro]) s_flag[lrow] = 1u;
  }
}
// Phase 3: the group's K' bytes and each row's flag byte, written once. A 16-byte line that lies
// inside the group is one store; the lines at the two edges are shared with the neighbouring groups
// (or end the matrix) and take byte stores of the group's own cells only.
KPE_SPLICE_DEV void splice_write(const SpliceGroup& G, uint32_t t, const uint8_t* s_o, const uint32_t* s_flag, uint8_t* out,
                                 uint8_t* flags) {
  for (uint64_t c0 = G.o.a0 + t * 16u; c0 < G.o.b1; c0 += 256u * 16u) {
    const uint32_t off = (uint32_t)(c0 - G.o.a0);
    if (c0 >= G.o.b0 && c0 + 16u <= G.o.b1) {
      uint32_t w[4];
      splice_lds_load16(s_o + off, w);
      splice_store16(out + c0, w);
    } else {
      const uint32_t lo = c0 < G.o.b0 ? G.o.skew : 0u;
      const uint32_t hi = G.o.b1 - c0 < 16u ? (uint32_t)(G.o.b1 - c0) : 16u;
      for (uint32_t k = lo; k < hi; ++k) out[c0 + k] = s_o[off + k];
    }
  }
  for (uint32_t i = t; i < G.rows; i += 256u) flags[G.r0 + i] = s_flag[i] ? 1u : 0u;
}
