// Gathering kept results across corpora (kpe_results_gather): row k of the output is row pairs[2k + 1]
// of source pairs[2k], for an N x R verdict matrix (R bytes per row) and for the fingerprints (8 bytes
// per row). The sources' base pointers come from a table in device memory, so one launch serves any
// number of sources. Included by results.hip (the bodies of kpe_results_gather_kernel and
// kpe_fp_gather_pairs_kernel) and by scripts/corpus_gather_check.cpp, which runs the same text lane by
// lane on the host under ASan / UBSan over buffers of exactly N x R and npairs x R bytes. The includer
// defines
//   KPE_GA_FN, KPE_GA_DEV   qualifiers of the arithmetic (the launcher uses it too) and of the bodies
//   ga_load4(p)             the 4 bytes at p, p 4-byte aligned
//   ga_store4(p, w)         w to the 4 bytes at p, p 4-byte aligned
//
// The output's npairs x R bytes are cut into one contiguous range per block, every range but the
// last a multiple of 16 bytes, so each block writes whole aligned words and only the matrix's last
// word can be partial (byte stores). A lane takes one output word at a time: its row and column from
// one division, the source row's address from the pair, then four byte loads that step into the next
// pair where the row ends (R < 4: more than once), or one word load when the four bytes lie in one
// source row at an aligned address. Every output byte is written once; nothing is read outside a
// listed row's R bytes.
constexpr uint32_t kGaLanes = 256;
constexpr uint32_t kGaGrid = 2048;       // most blocks (8 per CU)
constexpr uint32_t kGaMinSpan = 4096;    // bytes: a block's range is at least one word per lane, four times over

struct GaRange {
  uint64_t b0, b1;
};
// blocks of a launch over `total` bytes, and block b's range
KPE_GA_FN uint32_t ga_grid(uint64_t total) {
  const uint64_t g = (total + kGaMinSpan - 1u) / kGaMinSpan;
  return g < 1u ? 1u : (g > kGaGrid ? kGaGrid : (uint32_t)g);
}
KPE_GA_FN GaRange ga_range(uint64_t total, uint32_t grid, uint32_t b) {
  const uint64_t span = ((total + grid - 1u) / grid + 15u) & ~(uint64_t)15u;
  GaRange G;
  G.b0 = (uint64_t)b * span < total ? (uint64_t)b * span : total;
  G.b1 = G.b0 + span < total ? G.b0 + span : total;
  return G;
}

// Lane t of kGaLanes: the words of the block's range. out is 4-byte aligned.
KPE_GA_DEV void ga_copy(const GaRange& G, uint32_t t, const uint8_t* const* tab, const uint64_t* pairs, uint32_t R,
                        uint8_t* out) {
  for (uint64_t p = G.b0 + 4u * (uint64_t)t; p < G.b1; p += 4u * (uint64_t)kGaLanes) {
    const uint32_t cnt = G.b1 - p < 4u ? (uint32_t)(G.b1 - p) : 4u;  // < 4: the matrix's last word alone
    uint64_t k = p / R;
    uint32_t col = (uint32_t)(p - k * R);
    const uint8_t* src = tab[pairs[2u * k]] + pairs[2u * k + 1u] * R;
    uint32_t w = 0;
    if (cnt == 4u && col + 4u <= R && (((uintptr_t)(src + col)) & 3u) == 0u) {
      w = ga_load4(src + col);
    } else {
      for (uint32_t j = 0; j < cnt; ++j) {
        if (col == R) {  // the next output row: its own pair
          ++k, col = 0;
          src = tab[pairs[2u * k]] + pairs[2u * k + 1u] * R;
        }
        w |= (uint32_t)src[col++] << (8u * j);
      }
    }
    if (cnt == 4u) {
      ga_store4(out + p, w);
    } else {
      for (uint32_t j = 0; j < cnt; ++j) out[p + j] = (uint8_t)(w >> (8u * j));
    }
  }
}

// The fingerprint form: one 8-byte load and store per row.
KPE_GA_DEV void ga_fp(uint64_t k, const uint64_t* const* tab, const uint64_t* pairs, uint64_t* out) {
  out[k] = tab[pairs[2u * k]][pairs[2u * k + 1u]];
}
