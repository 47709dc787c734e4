// Report detail of a row list (kpe_fetch_report_rows): over the compact nrows x R verdict matrix of
// the listed rows, the cells whose report entry needs detail of each kind (check mask word, condition
// trace words, pattern record) and that detail, gathered through rows[]. include/kpe.h states the
// formats. Included by results.hip (the bodies of kpe_report_need_count_kernel and
// kpe_report_need_scatter_kernel) and by scripts/report_rows_check.cpp, which runs the same text lane
// by lane on the host under ASan / UBSan over buffers of exactly nrows x R bytes, N x R words,
// N x nmsg words and cap entries. The includer defines
//   KPE_RR_FN, KPE_RR_DEV      qualifiers of the arithmetic and of the per-lane phases
//   rr_load16(p, cnt, w)       cells [p, p + cnt) into w[4], cells past cnt zero; cnt <= 16 and p
//                              16-byte aligned (one 16-byte load when cnt == 16)
// and, before this file, KpeRrSrc / KpeRrOut (kernels_abi.h).
//
// The compact matrix is read as a flat array in tiles of 256 lanes x 16 cells, as the selection
// kernels read the whole matrix; a lane's first column is one `flat % R`, then increment-and-wrap.
// need: three R-byte tables, [mask][cond][pattern], in the KPE_SEL convention; no table selects
// KPE_NA, so a word of four NA cells (most of a wide matrix) is passed over. Kind k of a tile has
// its count at tile_counts[k * ntiles + tile]: one scan over the 3 * ntiles counts gives every
// kind's offsets (kind k's base is offs[k * ntiles], its end offs[(k + 1) * ntiles]).
constexpr uint32_t kRrTile = 4096;
constexpr uint32_t kRrKinds = 3;  // 0 mask, 1 cond, 2 pattern

KPE_RR_FN uint32_t rr_mod(uint64_t f, uint32_t R) { return (f >> 32) == 0 ? (uint32_t)f % R : (uint32_t)(f % R); }
KPE_RR_FN uint64_t rr_div(uint64_t f, uint32_t R) { return (f >> 32) == 0 ? (uint64_t)((uint32_t)f / R) : f / R; }
// column k <= 4 cells after column col
KPE_RR_FN uint32_t rr_col_add(uint32_t col, uint32_t k, uint32_t R) {
  col += k;
  return col < R ? col : (R >= k ? col - R : col % R);
}
// the lane's first cell of a tile and how many of its 16 cells lie in the matrix
KPE_RR_FN uint64_t rr_lane_first(uint64_t tile, uint32_t t) { return tile * kRrTile + t * 16u; }
KPE_RR_FN uint32_t rr_lane_cnt(uint64_t cells, uint64_t f) {
  return f >= cells ? 0u : (cells - f < 16u ? (uint32_t)(cells - f) : 16u);
}

// m[k] bit j: cell f + j needs detail of kind k. Cells past the matrix are never read or selected.
KPE_RR_DEV void rr_lane_hits(const uint8_t* v, uint64_t cells, uint32_t R, uint64_t tile, uint32_t t, const uint8_t* need,
                             uint32_t* m) {
  m[0] = m[1] = m[2] = 0u;
  const uint64_t f = rr_lane_first(tile, t);
  const uint32_t cnt = rr_lane_cnt(cells, f);
  if (!cnt) return;
  uint32_t w[4];
  rr_load16(v + f, cnt, w);
  uint32_t col = rr_mod(f, R);
#pragma unroll
  for (uint32_t q = 0; q < 4u; ++q) {
    if (w[q] == 0u) {
      col = rr_col_add(col, 4u, R);
      continue;
    }
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
      const uint32_t k = 4u * q + j;
      const uint32_t x = (w[q] >> (8u * j)) & 0xFFu;
      if (k < cnt && x != 0u && x < 8u) {
        m[0] |= ((need[col] >> x) & 1u) << k;
        m[1] |= ((need[R + col] >> x) & 1u) << k;
        m[2] |= ((need[2u * R + col] >> x) & 1u) << k;
      }
      col = col + 1u == R ? 0u : col + 1u;
    }
  }
}

// a tile is scattered when some kind has a hit in it below that kind's cap
KPE_RR_FN bool rr_tile_live(const uint64_t* o0, const uint64_t* o1, const KpeRrOut& O) {
  return (o0[0] != o1[0] && o0[0] < O.mask_cap) || (o0[1] != o1[1] && o0[1] < O.cond_cap) ||
         (o0[2] != o1[2] && o0[2] < O.pattern_cap);
}

// The lane's hits, from output slot o[k] of kind k on; slots at or past a cap are not written. The
// payload of compact cell (i, r) comes from row rows[i] of the corpus's matrices.
KPE_RR_DEV void rr_lane_scatter(uint64_t f, const uint32_t* m, const uint64_t* o, uint32_t R, const KpeRrSrc& S,
                                const KpeRrOut& O) {
  uint64_t om = o[0], oc = o[1], op = o[2];
  for (uint32_t any = m[0] | m[1] | m[2]; any; any &= any - 1u) {
    const uint32_t k = (uint32_t)__builtin_ctz(any);
    const uint64_t cell = f + k;
    const uint64_t i = rr_div(cell, R);
    const uint32_t r = (uint32_t)(cell - i * R);
    const uint64_t row = S.rows[i];
    if ((m[0] >> k) & 1u) {
      if (om < O.mask_cap) {
        O.mask_cells[om] = cell;
        O.mask_words[om] = S.masks[row * R + r];
      }
      ++om;
    }
    if ((m[1] >> k) & 1u) {
      if (oc < O.cond_cap) {
        const uint32_t e = S.slot[r];
        const uint32_t* src = S.mtrace + row * S.nmsg + KPE_RR_SLOT_FIRST(e);
        O.cond_cells[oc] = cell;
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) O.cond_words[oc * 4u + q] = q < KPE_RR_SLOT_WIDTH(e) ? src[q] : 0u;
      }
      ++oc;
    }
    if ((m[2] >> k) & 1u) {
      if (op < O.pattern_cap) {
        O.pattern_cells[op] = cell;
        O.pattern_abs[op] = row * R + r;
      }
      ++op;
    }
  }
}
