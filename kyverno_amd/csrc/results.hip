// Result kernels (gfx950): what runs over the finished verdict matrix, or patches it.
//  kpe_count_kernel      — per-rule status histogram (the CLI totals of
//                          cmd/cli/kubectl-kyverno/processor/result.go:34-68); fetch time.
//  kpe_fill_rows_kernel, kpe_apply_one_kernel — rows past an encoding limit, applyRules: One.
//  kpe_retire_rows_kernel — retired rows (kpe_corpus_retire_rows): no response, last of all.
//  kpe_delta_pairs_kernel, kpe_pair_rows_kernel, kpe_fp_pairs_kernel — a delta corpus's rows against
//                          the kept rows of another corpus they replace (kpe_changed_pairs[_fp]).
//  kpe_pack3_kernel      — the 3-bit verdict exchange.
//  kpe_select_*_kernel, kpe_row_summary_kernel — sparse result fetch.
//  kpe_ns_count*_kernel  — per-namespace rule counts.
//  kpe_delta_*_kernel, kpe_gather_rows_kernel — result deltas against a kept matrix.
//  kpe_splice_kernel     — a policy edit's columns spliced into the kept matrix (kpe_results_splice).
//  kpe_row_fp_kernel, kpe_fp_diff_kernel, kpe_fp_gather_kernel — row fingerprints and their compare.
//  kpe_results_gather_kernel, kpe_fp_gather_pairs_kernel — kept rows of several corpora gathered into
//                          another's kept matrix / fingerprints (kpe_results_gather).
//  kpe_report_need_count_kernel, kpe_report_need_scatter_kernel, kpe_fe_words_gather_kernel — the
//                          report detail of a row list (check mask words, condition trace words,
//                          pattern cells).
// None of them reads a program or runs a VM.
#include "kernels_common.h"

// Per-rule status histogram of a row-major N x R verdict matrix (8 slots per rule: the
// kpe_verdict codes). Each wave takes 64 rows at a time; per rule, one ballot per status,
// lane 0 accumulates in LDS; one 64-bit global add per (rule, status) and block at the end.
__global__ void __launch_bounds__(256) kpe_count_kernel(const uint8_t* v, int64_t n, uint32_t R, uint32_t r0,
                                                        uint32_t rn, unsigned long long* out) {
  extern __shared__ uint32_t hist[];  // rules [r0, r0 + rn) x 8
  const uint32_t t = threadIdx.x, lane = t & 63u;
  for (uint32_t i = t; i < rn * 8; i += 256) hist[i] = 0;
  __syncthreads();
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + (t >> 6); tile * 64 < n; tile += nw) {
    const int64_t row = tile * 64 + lane;
    const bool live = row < n;
    for (uint32_t r = 0; r < rn; ++r) {
      const uint32_t c = live ? v[row * R + r0 + r] : 0u;
#pragma unroll
      for (uint32_t s = 1; s < 8; ++s) {
        const uint32_t k = (uint32_t)__popcll(__ballot(c == s));
        if (lane == 0 && k) atomicAdd(&hist[r * 8 + s], k);
      }
    }
  }
  __syncthreads();
  for (uint32_t i = t; i < rn * 8; i += 256)
    if (hist[i]) atomicAdd(&out[(size_t)r0 * 8 + i], (unsigned long long)hist[i]);
}
extern "C" hipError_t kpe_launch_count(const uint8_t* verdicts, int64_t n, uint32_t R, unsigned long long* out,
                                       hipStream_t s) {
  if (R == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(out, 0, (size_t)R * 8 * 8, s);
  if (e != hipSuccess || n == 0) return e;
  const int64_t waves = (n + 63) / 64;
  const uint32_t grid = (uint32_t)std::min<int64_t>((waves + 3) / 4, 1024);
  for (uint32_t r0 = 0; r0 < R; r0 += 1536) {  // <= 48 KiB of LDS histogram per launch
    const uint32_t rn = std::min<uint32_t>(1536, R - r0);
    hipLaunchKernelGGL(kpe_count_kernel, dim3(grid), dim3(256), (size_t)rn * 8 * 4, s, verdicts, n, R, r0, rn, out);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// Rows past a per-resource encoding limit (Corpus::limit_rows): every cell undecided.
__global__ void __launch_bounds__(256) kpe_fill_rows_kernel(uint8_t* verdicts, uint32_t R, const uint32_t* rows,
                                                            uint32_t nrows, uint8_t value) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (uint64_t)nrows * R) verdicts[(size_t)rows[i / R] * R + i % R] = value;
}
extern "C" hipError_t kpe_launch_fill_rows(uint8_t* verdicts, uint32_t R, const uint32_t* rows, uint32_t nrows,
                                           uint8_t value, hipStream_t s) {
  const uint64_t cells = (uint64_t)nrows * R;
  if (cells == 0) return hipSuccess;
  hipLaunchKernelGGL(kpe_fill_rows_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, verdicts, R, rows,
                     nrows, value);
  return hipGetLastError();
}
// applyRules: One (pkg/engine/validation.go:75-77: stop after the first rule whose response is
// pass or fail, RulesAppliedCount) over the final verdicts: cells after an applied rule of the
// policy give no response; after an undecided cell they are undecided (unless unmatched).
__global__ void __launch_bounds__(256) kpe_apply_one_kernel(uint8_t* verdicts, uint32_t* masks, uint32_t n, uint32_t R,
                                                            const uint2* segs, uint32_t nsegs) {
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  uint8_t* row = verdicts + (size_t)r * R;
#pragma unroll 1
  for (uint32_t s = 0; s < nsegs; ++s) {
    const uint2 sg = segs[s];
    uint32_t state = 0;  // 0 open, 1 applied, 2 an earlier cell undecided
#pragma unroll 1
    for (uint32_t i = sg.x; i < sg.y; ++i) {
      const uint32_t v = row[i];
      if (state == 1u) {
        if (v != KPE_NA_) {
          row[i] = KPE_NA_;
          if (masks) masks[(size_t)r * R + i] = 0u;
        }
      } else if (state == 2u) {
        if (v != KPE_NA_) row[i] = KPE_UNDECIDED_;
      } else if (v == KPE_PASS_ || v == KPE_FAIL_) {
        state = 1u;
      } else if (v == KPE_UNDECIDED_) {
        state = 2u;
      }
    }
  }
}
extern "C" hipError_t kpe_launch_apply_one(uint8_t* verdicts, uint32_t* masks, int64_t n, uint32_t R, const uint32_t* segs,
                                           uint32_t nsegs, hipStream_t s) {
  if (n <= 0 || nsegs == 0) return hipSuccess;
  hipLaunchKernelGGL(kpe_apply_one_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, verdicts, masks,
                     (uint32_t)n, R, reinterpret_cast<const uint2*>(segs), nsegs);
  return hipGetLastError();
}

// Retired rows (kpe_corpus_retire_rows): every cell KPE_NA, every check mask word 0, after every
// other kernel of the evaluation. A row is R contiguous bytes from byte row * R of a 4-byte aligned
// matrix: the bytes before the first aligned word (head, at most 3), whole words, the bytes after
// the last one (tail, at most 3). A row takes W = R / 4 + 2 work items (the head, R / 4 word slots,
// the tail) and, with masks, R more (one per mask word); a thread takes one item at a time. A row
// that ends before its first aligned word is all head.
__global__ void __launch_bounds__(256) kpe_retire_rows_kernel(uint8_t* verdicts, uint32_t* masks, uint32_t R,
                                                              const uint32_t* rows, uint32_t nrows) {
  const uint32_t W = R / 4u + 2u, per = W + (masks ? R : 0u);
  const uint64_t items = (uint64_t)nrows * per;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < items; i += (uint64_t)gridDim.x * 256u) {
    const uint64_t k = i / per;
    const uint32_t j = (uint32_t)(i - k * per);
    const uint64_t b0 = (uint64_t)rows[k] * R, b1 = b0 + R;
    if (j >= W) {
      masks[b0 + (j - W)] = 0u;
      continue;
    }
    const uint64_t up = (b0 + 3u) & ~(uint64_t)3u, dn = b1 & ~(uint64_t)3u;
    const uint64_t a = up < b1 ? up : b1;  // end of the head
    const uint64_t e = a > dn ? a : dn;    // end of the words
    if (j == 0u) {
      for (uint64_t b = b0; b < a; ++b) verdicts[b] = KPE_NA_;
    } else if (j == W - 1u) {
      for (uint64_t b = e; b < b1; ++b) verdicts[b] = KPE_NA_;
    } else {
      const uint64_t w = a + 4u * (uint64_t)(j - 1u);
      if (w + 4u <= e) *reinterpret_cast<uint32_t*>(verdicts + w) = 0u;  // KPE_NA_ x 4; w is a multiple of 4 here
    }
  }
}
static_assert(KPE_NA_ == 0, "a retired row's words are zero");
extern "C" hipError_t kpe_launch_retire_rows(uint8_t* verdicts, uint32_t* masks, uint32_t R, const uint32_t* rows,
                                             uint32_t nrows, hipStream_t s) {
  const uint64_t items = (uint64_t)nrows * (R / 4u + 2u + (masks ? R : 0u));
  if (!nrows || !R) return hipSuccess;
  const dim3 grid((unsigned)std::min<uint64_t>((items + 255u) / 256u, 1u << 16));
  hipLaunchKernelGGL(kpe_retire_rows_kernel, grid, dim3(256), 0, s, verdicts, masks, R, rows, nrows);
  return hipGetLastError();
}

// Verdict exchange (kpe_pack_verdicts): 3-bit cells, 10 per 32-bit word, row-major. One thread
// per output word; neighbouring threads read neighbouring 10-byte runs (HBM-bound).
__global__ void __launch_bounds__(256) kpe_pack3_kernel(const uint8_t* __restrict__ v, uint64_t cells,
                                                        uint32_t* __restrict__ out, uint64_t words) {
  const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (w >= words) return;
  const uint64_t c0 = w * 10u;
  uint32_t x = 0;
#pragma unroll
  for (uint32_t k = 0; k < 10u; ++k)
    if (c0 + k < cells) x |= (uint32_t)(v[c0 + k] & 7u) << (3u * k);
  out[w] = x;
}
extern "C" hipError_t kpe_launch_pack3(const uint8_t* v, uint64_t cells, uint32_t* out, hipStream_t s) {
  const uint64_t words = (cells + 9u) / 10u;
  if (!words) return hipSuccess;
  hipLaunchKernelGGL(kpe_pack3_kernel, dim3((unsigned)((words + 255u) / 256u)), dim3(256), 0, s, v, cells, out, words);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Sparse result fetch (kpe_select_cells, kpe_fetch_row_summaries): reductions of the verdict
// matrix read as a flat array of N x R bytes, 16 cells per lane with one 16-byte load (the matrix
// is a hipMalloc allocation, so a multiple of 16 from its base is aligned); a block tile is
// 256 x 16 = 4096 cells. A lane's tail is bounded by count: no byte past the range is read.
// Per-rule byte tables (the selection masks, the unscored flags) are staged in LDS up to
// kSelLdsRules rules and read from global memory past that.
constexpr uint32_t kSelTile = 4096;
constexpr uint32_t kSelLdsRules = 16384;
constexpr uint32_t kSelGrid = 2048;   // persistent blocks of the selection kernels (8 per CU: every wave slot)
constexpr uint32_t kSumRows = 1024;   // rows a block of the summary kernel counts at a time (24 KiB of LDS)
constexpr uint32_t kSumGrid = 1536;   // persistent blocks of the summary kernel (6 per CU: what its LDS allows)

namespace {
struct Cells16 {
  uint32_t w[4];
  __device__ __forceinline__ uint32_t at(uint32_t k) const {  // k: compile-time after unrolling
    return (w[k >> 2] >> (8u * (k & 3u))) & 0xFFu;
  }
  __device__ __forceinline__ uint32_t at_dyn(uint32_t k) const {
    const uint64_t lo = (uint64_t)w[0] | ((uint64_t)w[1] << 32), hi = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
    return (uint32_t)((k < 8u ? lo >> (8u * k) : hi >> (8u * (k - 8u))) & 0xFFu);
  }
};
// cells [f, f + cnt) of the matrix, cnt <= 16, f a multiple of 16
__device__ __forceinline__ Cells16 load_cells(const uint8_t* __restrict__ v, uint64_t f, uint32_t cnt) {
  Cells16 c;
  if (cnt == 16u) {
    const uint4 q = *reinterpret_cast<const uint4*>(v + f);
    c.w[0] = q.x, c.w[1] = q.y, c.w[2] = q.z, c.w[3] = q.w;
  } else {
    c.w[0] = c.w[1] = c.w[2] = c.w[3] = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 15u; ++k)
      if (k < cnt) c.w[k >> 2] |= (uint32_t)v[f + k] << (8u * (k & 3u));
  }
  return c;
}
__device__ __forceinline__ uint32_t flat_col(uint64_t f, uint32_t R) {
  return (f >> 32) == 0 ? (uint32_t)f % R : (uint32_t)(f % R);
}
// column k <= 4 cells after column col
__device__ __forceinline__ uint32_t col_add(uint32_t col, uint32_t k, uint32_t R) {
  col += k;
  return col < R ? col : (R >= k ? col - R : col % R);
}
// bit k: cell f + k is selected (the cell's verdict v has bit v of its rule's mask set). skip_na
// (uniform: no rule selects KPE_NA): a word of four NA cells is passed over without its table
// reads; most cells of a wide matrix are NA. Cells past cnt are zero and never selected.
__device__ __forceinline__ uint32_t sel_hits(const Cells16& c, uint32_t cnt, uint32_t col, uint32_t R,
                                             const uint8_t* tbl, bool skip_na) {
  uint32_t m = 0;
#pragma unroll
  for (uint32_t w = 0; w < 4u; ++w) {
    if (skip_na && c.w[w] == 0u) {
      col = col_add(col, 4u, R);
      continue;
    }
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
      const uint32_t k = 4u * w + j;
      const uint32_t v = c.at(k);
      const uint32_t s = tbl[col];
      if (k < cnt && v < 8u && ((s >> v) & 1u)) m |= 1u << k;
      col = col + 1u == R ? 0u : col + 1u;
    }
  }
  return m;
}
// the block's per-rule byte table: staged in LDS (uniform branch), or the global one
template <bool LDS>
__device__ __forceinline__ const uint8_t* stage_table(const uint8_t* __restrict__ g, uint32_t R, uint8_t* lds) {
  if (!LDS) return g;
  for (uint32_t i = threadIdx.x; i < R; i += 256u) lds[i] = g[i];
  __syncthreads();
  return lds;
}
}  // namespace

// Pass 1: selected cells per tile (popcount of each lane's 16-bit hit mask, block sum).
template <bool LDS>
__global__ void __launch_bounds__(256) kpe_select_count_kernel(const uint8_t* __restrict__ v, uint64_t cells, uint32_t R,
                                                               const uint8_t* __restrict__ sel, uint32_t skip_na,
                                                               uint32_t* __restrict__ tile_counts, uint64_t ntiles) {
  extern __shared__ uint8_t s_sel_tbl[];
  __shared__ uint32_t s_w[2][4];  // by tile parity: one barrier per tile
  const uint32_t t = threadIdx.x;
  const uint8_t* tbl = stage_table<LDS>(sel, R, s_sel_tbl);
  uint32_t par = 0;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x, par ^= 1u) {
    const uint64_t f = tile * kSelTile + t * 16u;
    const uint32_t cnt = f >= cells ? 0u : (cells - f < 16u ? (uint32_t)(cells - f) : 16u);
    uint32_t hits = 0;
    if (cnt) hits = __popc(sel_hits(load_cells(v, f, cnt), cnt, flat_col(f, R), R, tbl, skip_na != 0u));
    const uint32_t inc = wave_incl_scan(hits);
    if ((t & 63u) == 63u) s_w[par][t >> 6] = inc;
    __syncthreads();
    if (t == 0) tile_counts[tile] = s_w[par][0] + s_w[par][1] + s_w[par][2] + s_w[par][3];
  }
}

// Pass 2: exclusive 64-bit scan of the tile counts, offs[ntiles] = the total. One block, 4096
// tiles per round (16 per thread, four 16-byte loads: tile_counts is 16-byte aligned and padded to
// a multiple of four entries).
__global__ void __launch_bounds__(256) kpe_select_scan_kernel(const uint32_t* __restrict__ tile_counts,
                                                              uint64_t* __restrict__ offs, uint64_t ntiles) {
  __shared__ uint32_t s_w[4];
  const uint32_t t = threadIdx.x;
  uint64_t carry = 0;
  for (uint64_t base = 0; base < ntiles; base += 4096u) {
    const uint64_t i0 = base + t * 16u;
    uint32_t c[16], sum = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
      uint4 x = make_uint4(0u, 0u, 0u, 0u);
      if (i0 + 4u * q < ntiles) x = *reinterpret_cast<const uint4*>(tile_counts + i0 + 4u * q);
      c[4u * q] = x.x, c[4u * q + 1u] = x.y, c[4u * q + 2u] = x.z, c[4u * q + 3u] = x.w;
    }
#pragma unroll
    for (uint32_t k = 0; k < 16u; ++k) {
      if (i0 + k >= ntiles) c[k] = 0u;  // the padding
      sum += c[k];
    }
    const uint32_t inc = wave_incl_scan(sum);  // <= 256 x 16 x 4096: 32 bits hold a round
    if ((t & 63u) == 63u) s_w[t >> 6] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4u; ++w) {
      if (w < (t >> 6)) before += s_w[w];
      all += s_w[w];
    }
    uint64_t o = carry + before + (inc - sum);
#pragma unroll
    for (uint32_t k = 0; k < 16u; ++k) {
      if (i0 + k < ntiles) offs[i0 + k] = o;
      o += c[k];
    }
    carry += all;
    __syncthreads();
  }
  if (t == 0) offs[ntiles] = carry;
}

// Pass 3: the hit masks again; a lane's first output slot is its tile's offset + the waves before
// it (LDS) + the lanes before it (DPP scan). Only slots below cap are written. Tiles without a
// selected cell, and tiles that start at or past cap, are not read.
template <bool LDS>
__global__ void __launch_bounds__(256) kpe_select_scatter_kernel(const uint8_t* __restrict__ v, uint64_t cells, uint32_t R,
                                                                 const uint8_t* __restrict__ sel, uint32_t skip_na,
                                                                 const uint64_t* __restrict__ offs, uint64_t ntiles,
                                                                 uint64_t cap, uint64_t* __restrict__ out_cells,
                                                                 uint8_t* __restrict__ out_v) {
  extern __shared__ uint8_t s_sel_tbl[];
  __shared__ uint32_t s_w[4];
  const uint32_t t = threadIdx.x;
  const uint8_t* tbl = stage_table<LDS>(sel, R, s_sel_tbl);
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint64_t o0 = offs[tile], o1 = offs[tile + 1];  // uniform
    if (o0 == o1 || o0 >= cap) continue;
    const uint64_t f = tile * kSelTile + t * 16u;
    const uint32_t cnt = f >= cells ? 0u : (cells - f < 16u ? (uint32_t)(cells - f) : 16u);
    Cells16 c;
    uint32_t m = 0;
    if (cnt) {
      c = load_cells(v, f, cnt);
      m = sel_hits(c, cnt, flat_col(f, R), R, tbl, skip_na != 0u);
    }
    const uint32_t hits = __popc(m);
    const uint32_t inc = wave_incl_scan(hits);
    if ((t & 63u) == 63u) s_w[t >> 6] = inc;
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (uint32_t w = 0; w < 3u; ++w)
      if (w < (t >> 6)) before += s_w[w];
    uint64_t o = o0 + before + (inc - hits);
    while (m) {
      const uint32_t k = (uint32_t)__builtin_ctz(m);
      m &= m - 1u;
      if (o < cap) {
        out_cells[o] = f + k;
        if (out_v) out_v[o] = (uint8_t)c.at_dyn(k);
      }
      ++o;
    }
    __syncthreads();
  }
}

// CalculateSummary per resource (pkg/utils/report/results.go:39-55 over :89-135): rows
// [row0, row0 + nrows), 6 uint16 counters per row (pass, fail, warn, error, skip, undecided) as 3
// words. A block takes groups of rows_per_group whole rows (<= kSumRows, about one tile of bytes),
// reads their contiguous bytes with the aligned 16-byte loads (cells before the group's first byte
// are skipped by index) and counts each lane's cells of one row in a register (5 bits per counter)
// before adding them to the row's LDS counters; each row is written once. With R >= 16 a lane's 16
// cells lie in at most two rows: two registers, no branch per cell, and words of four KPE_NA cells
// (most of a wide matrix) are passed over. unscored[r] != 0: a FAIL of rule r counts as warn
// (results.go:131-133).
template <bool LDS>
__global__ void __launch_bounds__(256) kpe_row_summary_kernel(const uint8_t* __restrict__ v, uint32_t R, uint64_t row0,
                                                              uint64_t nrows, uint32_t rows_per_group,
                                                              const uint8_t* __restrict__ unscored,
                                                              uint32_t* __restrict__ out) {
  extern __shared__ uint8_t s_sel_tbl[];
  __shared__ uint32_t s_cnt[kSumRows * 6u];
  const uint32_t t = threadIdx.x;
  const uint8_t* tbl = stage_table<LDS>(unscored, R, s_sel_tbl);
  const uint64_t ngroups = (nrows + rows_per_group - 1u) / rows_per_group;
  // a lane's counts of one row (5 bits per counter, at most 16 cells) into the row's LDS counters
  auto flush = [&](uint32_t acc, uint32_t lrow) {
    while (acc) {
      const uint32_t s = (uint32_t)__builtin_ctz(acc) / 5u;
      atomicAdd(&s_cnt[lrow * 6u + s], (acc >> (5u * s)) & 31u);
      acc &= ~(31u << (5u * s));
    }
  };
  // the counter increment of verdict code x of rule col (0: not counted). Code -> counter + 1:
  // PASS, FAIL (or warn), WARN, ERROR, SKIP, -, UNDECIDED
  auto cell_inc = [&](uint32_t x, uint32_t col) -> uint32_t {
    const uint32_t lut = 0x60543210u + (tbl[col] ? 0x100u : 0u);
    const uint32_t slot = x < 8u ? (lut >> (4u * x)) & 15u : 0u;
    return (1u << (5u * slot)) >> 5;
  };
  for (uint64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const uint64_t r0 = g * rows_per_group;  // relative to row0
    const uint32_t rn = nrows - r0 < rows_per_group ? (uint32_t)(nrows - r0) : rows_per_group;
    for (uint32_t i = t; i < rn * 6u; i += 256u) s_cnt[i] = 0u;
    __syncthreads();
    const uint64_t g0 = (row0 + r0) * R, g1 = g0 + (uint64_t)rn * R;  // the group's bytes: < 2^32 of them
    for (uint64_t c0 = (g0 & ~(uint64_t)15u) + t * 16u; c0 < g1; c0 += kSelTile) {
      const uint32_t cnt = g1 - c0 < 16u ? (uint32_t)(g1 - c0) : 16u;
      const uint32_t k0 = c0 < g0 ? (uint32_t)(g0 - c0) : 0u;  // c0 may start up to 15 cells before the group
      if (k0 >= cnt) continue;
      const Cells16 c = load_cells(v, c0, cnt);
      const uint32_t rel = (uint32_t)(c0 + k0 - g0);
      uint32_t lrow = rel / R, col = rel - lrow * R;
      if (R >= 16u) {  // uniform: cell k is in row lrow, or in lrow + 1 once its column wraps
        uint32_t acc0 = 0, acc1 = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4u; ++w) {
          if (c.w[w] == 0u) continue;
#pragma unroll
          for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t k = 4u * w + j;
            const uint32_t ck = col + (k >= k0 ? k - k0 : 0u);  // < 2 R
            const bool next = ck >= R;
            const uint32_t inc = (k >= k0 && k < cnt) ? cell_inc(c.at(k), next ? ck - R : ck) : 0u;
            acc0 += next ? 0u : inc;
            acc1 += next ? inc : 0u;
          }
        }
        flush(acc0, lrow);
        flush(acc1, lrow + 1u);  // non-zero only when a counted cell lies in that row
      } else {
        uint32_t acc = 0;
#pragma unroll
        for (uint32_t k = 0; k < 16u; ++k) {
          if (k >= k0 && k < cnt) {
            acc += cell_inc(c.at(k), col);
            if (++col == R) {
              flush(acc, lrow);
              acc = 0, col = 0, ++lrow;
            }
          }
        }
        flush(acc, lrow);
      }
    }
    __syncthreads();
    for (uint32_t i = t; i < rn * 3u; i += 256u) out[r0 * 3u + i] = s_cnt[2u * i] | (s_cnt[2u * i + 1u] << 16);
    __syncthreads();
  }
}

// tile_counts: ntiles words, tile_offs: ntiles + 1 offsets (the last one is the total)
// na_selected: some rule's mask selects KPE_NA
extern "C" hipError_t kpe_launch_select_count(const uint8_t* v, uint64_t cells, uint32_t R, const uint8_t* sel,
                                              int na_selected, uint32_t* tile_counts, uint64_t* tile_offs,
                                              hipStream_t s) {
  if (!cells || !R) return hipSuccess;
  const uint64_t ntiles = (cells + kSelTile - 1u) / kSelTile;
  const dim3 grid((unsigned)std::min<uint64_t>(ntiles, kSelGrid));
  const uint32_t skip_na = na_selected ? 0u : 1u;
  if (R <= kSelLdsRules)
    hipLaunchKernelGGL(kpe_select_count_kernel<true>, grid, dim3(256), (size_t)R, s, v, cells, R, sel, skip_na,
                       tile_counts, ntiles);
  else
    hipLaunchKernelGGL(kpe_select_count_kernel<false>, grid, dim3(256), 0, s, v, cells, R, sel, skip_na, tile_counts,
                       ntiles);
  hipLaunchKernelGGL(kpe_select_scan_kernel, dim3(1), dim3(256), 0, s, tile_counts, tile_offs, ntiles);
  return hipGetLastError();
}
// out_cells / out_v (may be NULL): at least min(total, cap) entries
extern "C" hipError_t kpe_launch_select_scatter(const uint8_t* v, uint64_t cells, uint32_t R, const uint8_t* sel,
                                                int na_selected, const uint64_t* tile_offs, uint64_t cap,
                                                uint64_t* out_cells, uint8_t* out_v, hipStream_t s) {
  if (!cells || !R || !cap) return hipSuccess;
  const uint64_t ntiles = (cells + kSelTile - 1u) / kSelTile;
  const dim3 grid((unsigned)std::min<uint64_t>(ntiles, kSelGrid));
  const uint32_t skip_na = na_selected ? 0u : 1u;
  if (R <= kSelLdsRules)
    hipLaunchKernelGGL(kpe_select_scatter_kernel<true>, grid, dim3(256), (size_t)R, s, v, cells, R, sel, skip_na,
                       tile_offs, ntiles, cap, out_cells, out_v);
  else
    hipLaunchKernelGGL(kpe_select_scatter_kernel<false>, grid, dim3(256), 0, s, v, cells, R, sel, skip_na, tile_offs,
                       ntiles, cap, out_cells, out_v);
  return hipGetLastError();
}
// out: 3 words per row of [row0, row0 + nrows); R <= 65535 (the counters are 16 bits wide)
extern "C" hipError_t kpe_launch_row_summary(const uint8_t* v, uint32_t R, uint64_t row0, uint64_t nrows,
                                             const uint8_t* unscored, uint32_t* out, hipStream_t s) {
  if (!nrows || !R) return hipSuccess;
  const uint32_t rpg = std::max<uint32_t>(1u, std::min<uint32_t>(kSumRows, kSelTile / R));
  const uint64_t ngroups = (nrows + rpg - 1u) / rpg;
  const dim3 grid((unsigned)std::min<uint64_t>(ngroups, kSumGrid));
  if (R <= kSelLdsRules)
    hipLaunchKernelGGL(kpe_row_summary_kernel<true>, grid, dim3(256), (size_t)R, s, v, R, row0, nrows, rpg, unscored, out);
  else
    hipLaunchKernelGGL(kpe_row_summary_kernel<false>, grid, dim3(256), 0, s, v, R, row0, nrows, rpg, unscored, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Result deltas (kpe_changed_rows, kpe_delta_transitions): the new verdict matrix of a resident
// corpus against the one kpe_results_keep kept, column r of the new one against column tab[r] of
// the kept one. The flag pass (delta.inl, shared with scripts/delta_check.cpp) writes one byte per
// row; the row list is the selection chain above run over the flag bytes as an N x 1 matrix
// (kpe_launch_select_count / _scatter with the mask KPE_SEL(1)); kpe_gather_rows_kernel copies the
// listed rows. No global atomics on that path: a row's byte is written once, by the block that
// owns the row's group.
#define KPE_DELTA_FN __host__ __device__ __forceinline__
#define KPE_DELTA_DEV __device__ __forceinline__
namespace {
__device__ __forceinline__ void delta_load16(const uint8_t* __restrict__ p, uint32_t cnt, uint32_t* w) {
  const Cells16 c = load_cells(p, 0, cnt);
  w[0] = c.w[0], w[1] = c.w[1], w[2] = c.w[2], w[3] = c.w[3];
}
__device__ __forceinline__ void delta_store16(uint8_t* p, const uint32_t* w) {
  *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
}
#include "delta.inl"
}  // namespace
constexpr uint32_t kDeltaGrid = 2048;       // persistent blocks of the flag pass (8 per CU)
constexpr uint32_t kDeltaTransRules = 192;  // rules per launch of the transition kernel: 64 words each, 48 KiB

// All LDS is dynamic, so its base is 16-byte aligned for the staging stores (delta_lds).
__global__ void __launch_bounds__(256) kpe_delta_flags_kernel(const uint8_t* __restrict__ vnew,
                                                              const uint8_t* __restrict__ vold, uint64_t n, uint32_t Rn,
                                                              uint32_t Ro, uint32_t rpg, const uint32_t* __restrict__ tab,
                                                              const uint8_t* __restrict__ unmapped,
                                                              uint8_t* __restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_delta[];
  const uint32_t t = threadIdx.x;
  const DeltaLds L = delta_lds(Rn, Ro, rpg);
  uint8_t* s_old = s_delta;
  uint32_t* s_flag = reinterpret_cast<uint32_t*>(s_delta + L.flag_off);
  uint32_t* s_tab = reinterpret_cast<uint32_t*>(s_delta + L.tab_off);
  uint8_t* s_unm = s_delta + L.unm_off;
  for (uint32_t i = t; i < Rn; i += 256u) s_tab[i] = tab[i];
  if (unmapped)
    for (uint32_t i = t; i < Ro; i += 256u) s_unm[i] = unmapped[i];
  const uint64_t ngroups = (n + rpg - 1u) / rpg;
  for (uint64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const DeltaGroup G = delta_group(g, n, Rn, Ro, rpg);
    delta_stage(G, t, vold, s_old, s_flag);
    __syncthreads();  // the first one also covers the tables
    delta_compare(G, t, vnew, Rn, Ro, s_tab, s_old, s_flag);
    if (unmapped) delta_sweep(G, t, Ro, s_unm, s_old, s_flag);  // uniform
    __syncthreads();
    delta_write(G, t, s_flag, flags);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) kpe_gather_rows_kernel(const uint8_t* __restrict__ v, uint32_t R,
                                                              const uint64_t* __restrict__ rows, uint64_t bytes,
                                                              uint8_t* __restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < bytes; i += (uint64_t)gridDim.x * 256u) {
    const uint64_t k = i / R;
    out[i] = v[rows[k] * R + (i - k * R)];
  }
}

// Per new column r of [r0, r0 + rn) the 8 x 8 table of (kept code, new code) over all rows, after
// kpe_count_kernel: a wave takes 64 rows at a time; per rule the lanes' (old, new) pairs are
// counted with one ballot per distinct pair of the wave (a few), lane 0 accumulates in LDS; one
// 64-bit global add per non-zero counter and block at the end. Codes are taken & 7 (the alphabet).
__global__ void __launch_bounds__(256) kpe_delta_trans_kernel(const uint8_t* __restrict__ vnew,
                                                              const uint8_t* __restrict__ vold, uint64_t n, uint32_t Rn,
                                                              uint32_t Ro, const uint32_t* __restrict__ tab, uint32_t r0,
                                                              uint32_t rn, unsigned long long* __restrict__ out) {
  extern __shared__ uint32_t s_trans[];  // rules [r0, r0 + rn) x 64
  const uint32_t t = threadIdx.x, lane = t & 63u;
  for (uint32_t i = t; i < rn * 64u; i += 256u) s_trans[i] = 0u;
  __syncthreads();
  const uint64_t nw = (uint64_t)gridDim.x * 4u;
  for (uint64_t tile = (uint64_t)blockIdx.x * 4u + (t >> 6); tile * 64u < n; tile += nw) {
    const uint64_t row = tile * 64u + lane;
    const bool live = row < n;
    for (uint32_t r = 0; r < rn; ++r) {
      const uint32_t m = tab[r0 + r] & 0xFFFFu;  // uniform
      const uint32_t c = live ? vnew[row * Rn + r0 + r] & 7u : 0u;
      const uint32_t o = live && m != kDeltaNone ? vold[row * Ro + m] & 7u : 0u;
      const uint32_t key = o * 8u + c;
      uint64_t rem = __ballot(live);  // uniform
      while (rem) {
        const uint32_t k = (uint32_t)__shfl((int)key, (int)__builtin_ctzll(rem), 64);
        const uint64_t same = __ballot(live && key == k);
        if (lane == 0) atomicAdd(&s_trans[r * 64u + k], (uint32_t)__popcll(same));
        rem &= ~same;
      }
    }
  }
  __syncthreads();
  for (uint32_t i = t; i < rn * 64u; i += 256u)
    if (s_trans[i]) atomicAdd(&out[(size_t)r0 * 64u + i], (unsigned long long)s_trans[i]);
}

extern "C" uint32_t kpe_delta_max_rules(void) { return kDeltaMaxRules; }
extern "C" hipError_t kpe_launch_delta_flags(const uint8_t* vnew, const uint8_t* vold, uint64_t n, uint32_t Rn,
                                             uint32_t Ro, const uint32_t* tab, const uint8_t* unmapped, uint8_t* flags,
                                             hipStream_t s) {
  if (!n) return hipSuccess;
  if (Rn > kDeltaMaxRules || Ro > kDeltaMaxRules) return hipErrorInvalidValue;
  const uint32_t rpg = delta_rows_per_group(Rn, Ro);
  const uint64_t ngroups = (n + rpg - 1u) / rpg;
  const dim3 grid((unsigned)std::min<uint64_t>(ngroups, kDeltaGrid));
  hipLaunchKernelGGL(kpe_delta_flags_kernel, grid, dim3(256), (size_t)delta_lds(Rn, Ro, rpg).total, s, vnew, vold, n, Rn,
                     Ro, rpg, tab, unmapped, flags);
  return hipGetLastError();
}
extern "C" hipError_t kpe_launch_gather_rows(const uint8_t* v, uint32_t R, const uint64_t* rows, uint64_t nrows,
                                             uint8_t* out, hipStream_t s) {
  const uint64_t bytes = nrows * R;
  if (!bytes) return hipSuccess;
  const dim3 grid((unsigned)std::min<uint64_t>((bytes + 255u) / 256u, 1u << 20));
  hipLaunchKernelGGL(kpe_gather_rows_kernel, grid, dim3(256), 0, s, v, R, rows, bytes, out);
  return hipGetLastError();
}
extern "C" hipError_t kpe_launch_delta_transitions(const uint8_t* vnew, const uint8_t* vold, uint64_t n, uint32_t Rn,
                                                   uint32_t Ro, const uint32_t* tab, unsigned long long* out,
                                                   hipStream_t s) {
  if (Rn == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(out, 0, (size_t)Rn * 64 * 8, s);
  if (e != hipSuccess || n == 0) return e;
  const uint64_t waves = (n + 63u) / 64u;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((waves + 3u) / 4u, 1024);
  for (uint32_t r0 = 0; r0 < Rn; r0 += kDeltaTransRules) {
    const uint32_t rn = std::min<uint32_t>(kDeltaTransRules, Rn - r0);
    hipLaunchKernelGGL(kpe_delta_trans_kernel, dim3(grid), dim3(256), (size_t)rn * 64 * 4, s, vnew, vold, n, Rn, Ro, tab,
                       r0, rn, out);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// ---------------------------------------------------------------------------
// Policy edits on a kept result (kpe_results_splice): the new kept matrix K' from the kept one K and
// the evaluation E of the edited policies alone, column by column through a plan, and one flag
// byte per row by the rule of the flag pass above restricted to E's columns and the kept columns
// that vanish (splice.inl, shared with scripts/splice_check.cpp). One pass, N x (Ro + Rs + rn + 1)
// algorithmic bytes; the row list is the selection chain over the flag bytes (kpe_spliced_rows). No
// global atomics and no zeroing pass: a row's cells and its flag byte are written once, by the
// block that owns the row's group.
#define KPE_SPLICE_FN __host__ __device__ __forceinline__
#define KPE_SPLICE_DEV __device__ __forceinline__
namespace {
__device__ __forceinline__ void splice_load16(const uint8_t* __restrict__ p, uint32_t cnt, uint32_t* w) {
  const Cells16 c = load_cells(p, 0, cnt);
  w[0] = c.w[0], w[1] = c.w[1], w[2] = c.w[2], w[3] = c.w[3];
}
__device__ __forceinline__ void splice_store16(uint8_t* p, const uint32_t* w) {
  *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ void splice_lds_store16(uint8_t* p, const uint32_t* w) {
  *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ void splice_lds_load16(const uint8_t* p, uint32_t* w) {
  const uint4 q = *reinterpret_cast<const uint4*>(p);
  w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
}
#include "splice.inl"
}  // namespace
constexpr uint32_t kSpliceGrid = 2048;  // persistent blocks (8 per CU)

// All LDS is dynamic, so its base is 16-byte aligned for the staging stores (splice_lds).
__global__ void __launch_bounds__(256) kpe_splice_kernel(const uint8_t* __restrict__ kept, const uint8_t* __restrict__ sub,
                                                         uint64_t n, uint32_t Ro, uint32_t Rs, uint32_t rn, uint32_t rpg,
                                                         const uint32_t* __restrict__ col,
                                                         const uint8_t* __restrict__ unmapped, uint8_t* __restrict__ out,
                                                         uint8_t* __restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_splice[];
  const uint32_t t = threadIdx.x;
  const SpliceLds L = splice_lds(Ro, Rs, rn, rpg);
  uint8_t* s_k = s_splice;
  uint8_t* s_e = s_splice + L.e_off;
  uint8_t* s_o = s_splice + L.o_off;
  uint32_t* s_flag = reinterpret_cast<uint32_t*>(s_splice + L.flag_off);
  uint32_t* s_col = reinterpret_cast<uint32_t*>(s_splice + L.col_off);
  uint8_t* s_unm = s_splice + L.unm_off;
  for (uint32_t i = t; i < 2u * rn; i += 256u) s_col[i] = col[i];
  if (unmapped)
    for (uint32_t i = t; i < Ro; i += 256u) s_unm[i] = unmapped[i];
  const uint64_t ngroups = (n + rpg - 1u) / rpg;
  for (uint64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const SpliceGroup G = splice_group(g, n, Ro, Rs, rn, rpg);
    splice_stage(G, t, kept, sub, s_k, s_e, s_flag);
    __syncthreads();  // the first one also covers the tables
    splice_build(G, t, Ro, Rs, rn, s_col, s_k, s_e, s_o, s_flag);
    if (unmapped) splice_sweep(G, t, Ro, s_unm, s_k, s_flag);  // uniform
    __syncthreads();
    splice_write(G, t, s_o, s_flag, out, flags);
    __syncthreads();
  }
}

extern "C" uint32_t kpe_splice_rows_per_group(uint32_t Ro, uint32_t Rs, uint32_t rn) {
  return splice_rows_per_group(Ro, Rs, rn);
}
extern "C" uint32_t kpe_splice_grid(void) { return kSpliceGrid; }
extern "C" hipError_t kpe_launch_splice(const uint8_t* kept, const uint8_t* sub, uint64_t n, uint32_t Ro, uint32_t Rs,
                                        uint32_t rn, const uint32_t* col, const uint8_t* unmapped, uint8_t* out,
                                        uint8_t* flags, hipStream_t s) {
  if (!n) return hipSuccess;
  if (Ro > kSpliceMaxRules || Rs > kSpliceMaxRules || rn > kSpliceMaxRules) return hipErrorInvalidValue;
  const uint32_t rpg = splice_rows_per_group(Ro, Rs, rn);
  const uint64_t ngroups = (n + rpg - 1u) / rpg;
  const dim3 grid((unsigned)std::min<uint64_t>(ngroups, kSpliceGrid));
  hipLaunchKernelGGL(kpe_splice_kernel, grid, dim3(256), (size_t)splice_lds(Ro, Rs, rn, rpg).total, s, kept, sub, n, Ro, Rs,
                     rn, rpg, col, unmapped, out, flags);
  return hipGetLastError();
}

// Result deltas across corpora (kpe_changed_pairs): pair k = {new_row, old_row}, row new_row of the
// new matrix against row old_row of another corpus's kept one, by the rules of the flag pass above.
// A delta is small (thousands of pairs) and its rows are scattered: no staging of rows. The tables
// are staged in LDS; a wave takes one pair at a time, lanes over the columns, and lane 0 writes the
// pair's byte once. The changed pairs are the selection chain over those bytes, as for the rows.
__global__ void __launch_bounds__(256) kpe_delta_pairs_kernel(const uint8_t* __restrict__ vnew,
                                                              const uint8_t* __restrict__ vold,
                                                              const uint64_t* __restrict__ pairs, uint64_t npairs,
                                                              uint32_t Rn, uint32_t Ro, const uint32_t* __restrict__ tab,
                                                              const uint8_t* __restrict__ unmapped,
                                                              uint8_t* __restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_delta[];
  const uint32_t t = threadIdx.x, lane = t & 63u;
  uint32_t* s_tab = reinterpret_cast<uint32_t*>(s_delta);
  uint8_t* s_unm = s_delta + delta_up16(Rn * 4u);
  for (uint32_t i = t; i < Rn; i += 256u) s_tab[i] = tab[i];
  if (unmapped)
    for (uint32_t i = t; i < Ro; i += 256u) s_unm[i] = unmapped[i];
  __syncthreads();
  const uint64_t nw = (uint64_t)gridDim.x * 4u;
  for (uint64_t k = (uint64_t)blockIdx.x * 4u + (t >> 6); k < npairs; k += nw) {  // no barrier below
    const uint8_t* nr = vnew + pairs[2u * k] * Rn;
    const uint8_t* od = vold + pairs[2u * k + 1u] * Ro;
    bool ch = false;
    for (uint32_t r = lane; r < Rn; r += 64u) {
      const uint32_t x = nr[r], e = s_tab[r], m = e & 0xFFFFu;
      const uint32_t o = m != kDeltaNone ? (uint32_t)od[m] : 0u;
      ch = ch || x != o || (x < 8u && ((e >> (16u + x)) & 1u));
    }
    if (unmapped)  // uniform: a response in a kept column no new column names
      for (uint32_t o = lane; o < Ro; o += 64u) ch = ch || (s_unm[o] && od[o] != 0u);
    const bool any = __ballot(ch) != 0ull;
    if (lane == 0u) flags[k] = any ? 1u : 0u;
  }
}
// out[i] = the new row of pair idx[i]: the row list kpe_gather_rows_kernel takes
__global__ void __launch_bounds__(256) kpe_pair_rows_kernel(const uint64_t* __restrict__ pairs,
                                                            const uint64_t* __restrict__ idx, uint64_t m,
                                                            uint64_t* __restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256u)
    out[i] = pairs[2u * idx[i]];
}
extern "C" hipError_t kpe_launch_delta_pairs(const uint8_t* vnew, const uint8_t* vold, const uint64_t* pairs,
                                             uint64_t npairs, uint32_t Rn, uint32_t Ro, const uint32_t* tab,
                                             const uint8_t* unmapped, uint8_t* flags, hipStream_t s) {
  if (!npairs) return hipSuccess;
  if (Rn > kDeltaMaxRules || Ro > kDeltaMaxRules) return hipErrorInvalidValue;
  const dim3 grid((unsigned)std::min<uint64_t>((npairs + 3u) / 4u, kDeltaGrid));
  const size_t dyn = (size_t)delta_up16(Rn * 4u) + delta_up16(Ro) + 16u;
  hipLaunchKernelGGL(kpe_delta_pairs_kernel, grid, dim3(256), dyn, s, vnew, vold, pairs, npairs, Rn, Ro, tab, unmapped,
                     flags);
  return hipGetLastError();
}
extern "C" hipError_t kpe_launch_pair_rows(const uint64_t* pairs, const uint64_t* idx, uint64_t m, uint64_t* out,
                                           hipStream_t s) {
  if (!m) return hipSuccess;
  const dim3 grid((unsigned)std::min<uint64_t>((m + 255u) / 256u, 1u << 16));
  hipLaunchKernelGGL(kpe_pair_rows_kernel, grid, dim3(256), 0, s, pairs, idx, m, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Row fingerprints (kpe_fetch_row_fingerprints, kpe_fingerprints_keep, kpe_changed_rows_fp): 8 bytes
// per row, the shape of kpe_row_summary_kernel (fp.inl, shared with scripts/fp_check.cpp). The
// changed rows are kpe_fp_diff_kernel's byte per row through the selection chain as an N x 1
// matrix, like the delta flags; kpe_gather_rows_kernel and kpe_fp_gather_kernel copy what the
// listed rows need. No global atomics, no zeroing pass: a row's word is written once.
#define KPE_FP_FN __host__ __device__ __forceinline__
#define KPE_FP_DEV __device__ __forceinline__
namespace {
__device__ __forceinline__ void fp_load16(const uint8_t* __restrict__ p, uint32_t cnt, uint32_t* w) {
  const Cells16 c = load_cells(p, 0, cnt);
  w[0] = c.w[0], w[1] = c.w[1], w[2] = c.w[2], w[3] = c.w[3];
}
__device__ __forceinline__ void fp_lds_add(uint64_t* p, uint64_t x) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)x);
}
#include "fp.inl"
}  // namespace
constexpr uint32_t kFpGrid = 2048;  // persistent blocks (8 per CU where the LDS allows)

// tbl: [salts: R][msg_salts: R]. LDS: both tables staged in dynamic LDS (R <= kFpLdsRules); MASKS:
// the FAIL cells' mask words count (the verdict-only instance has no such load).
template <bool LDS, bool MASKS>
__global__ void __launch_bounds__(256) kpe_row_fp_kernel(const uint8_t* __restrict__ v, const uint32_t* __restrict__ masks,
                                                         uint32_t R, uint64_t row0, uint64_t nrows, uint32_t rpg,
                                                         const uint64_t* __restrict__ tbl_g, uint32_t msg_codes,
                                                         uint64_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_fp_dyn[];
  __shared__ uint64_t s_fp[kFpMaxRows];
  const uint32_t t = threadIdx.x;
  const uint64_t* tbl = tbl_g;
  if (LDS) {  // the first barrier of the loop covers the staging
    uint64_t* l = reinterpret_cast<uint64_t*>(s_fp_dyn);
    for (uint32_t i = t; i < 2u * R; i += 256u) l[i] = tbl_g[i];
    tbl = l;
  }
  const uint64_t ngroups = (nrows + rpg - 1u) / rpg;
  for (uint64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const FpGroup G = fp_group(g, row0, nrows, R, rpg);
    fp_clear(G, t, s_fp);
    __syncthreads();
    fp_accum<MASKS>(G, t, v, masks, R, tbl, msg_codes, s_fp);
    __syncthreads();
    fp_write(G, t, s_fp, out);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) kpe_fp_diff_kernel(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b,
                                                          uint64_t n, uint8_t* __restrict__ flags) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u)
    flags[i] = a[i] != b[i] ? 1u : 0u;
}
__global__ void __launch_bounds__(256) kpe_fp_gather_kernel(const uint64_t* __restrict__ fp,
                                                            const uint64_t* __restrict__ rows, uint64_t m,
                                                            uint64_t* __restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256u)
    out[i] = fp[rows[i]];
}

extern "C" hipError_t kpe_launch_row_fp(const uint8_t* v, const uint32_t* masks, uint32_t R, uint64_t row0,
                                        uint64_t nrows, const uint64_t* tbl, uint32_t msg_codes, uint64_t* out,
                                        hipStream_t s) {
  if (!nrows) return hipSuccess;
  if (!R || R > kFpMaxRules) return hipErrorInvalidValue;
  const uint32_t rpg = fp_rows_per_group(R);
  const uint64_t ngroups = (nrows + rpg - 1u) / rpg;
  const dim3 grid((unsigned)std::min<uint64_t>(ngroups, kFpGrid));
  const bool lds = R <= kFpLdsRules;
  const size_t dyn = lds ? (size_t)R * 16u : 0u;
#define KPE_FP_LAUNCH(L, M) \
  hipLaunchKernelGGL((kpe_row_fp_kernel<L, M>), grid, dim3(256), dyn, s, v, masks, R, row0, nrows, rpg, tbl, msg_codes, out)
  if (lds && masks) KPE_FP_LAUNCH(true, true);
  else if (lds) KPE_FP_LAUNCH(true, false);
  else if (masks) KPE_FP_LAUNCH(false, true);
  else KPE_FP_LAUNCH(false, false);
#undef KPE_FP_LAUNCH
  return hipGetLastError();
}
extern "C" hipError_t kpe_launch_fp_diff(const uint64_t* a, const uint64_t* b, uint64_t n, uint8_t* flags, hipStream_t s) {
  if (!n) return hipSuccess;
  const dim3 grid((unsigned)std::min<uint64_t>((n + 255u) / 256u, 1u << 16));
  hipLaunchKernelGGL(kpe_fp_diff_kernel, grid, dim3(256), 0, s, a, b, n, flags);
  return hipGetLastError();
}
extern "C" hipError_t kpe_launch_fp_gather(const uint64_t* fp, const uint64_t* rows, uint64_t m, uint64_t* out,
                                           hipStream_t s) {
  if (!m) return hipSuccess;
  const dim3 grid((unsigned)std::min<uint64_t>((m + 255u) / 256u, 1u << 16));
  hipLaunchKernelGGL(kpe_fp_gather_kernel, grid, dim3(256), 0, s, fp, rows, m, out);
  return hipGetLastError();
}

// The fingerprint form of kpe_delta_pairs_kernel (kpe_changed_pairs_fp): pair k = {new_row,
// old_row}; fp_out[k] = the fingerprint of row new_row (fp.inl's cell hash, summed over the row by
// the wave: lanes over the columns, then a butterfly of 64-bit adds), flags[k] = it differs from
// kept[old_row]. lds != 0: both salt tables staged in dynamic LDS (R <= kFpLdsRules).
template <bool MASKS>
__global__ void __launch_bounds__(256) kpe_fp_pairs_kernel(const uint8_t* __restrict__ v, const uint32_t* __restrict__ masks,
                                                           uint32_t R, const uint64_t* __restrict__ pairs, uint64_t npairs,
                                                           const uint64_t* __restrict__ tbl_g, uint32_t lds,
                                                           uint32_t msg_codes, const uint64_t* __restrict__ kept,
                                                           uint64_t* __restrict__ fp_out, uint8_t* __restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_fp_dyn[];
  const uint32_t t = threadIdx.x, lane = t & 63u;
  const uint64_t* tbl = tbl_g;
  if (lds) {  // uniform
    uint64_t* l = reinterpret_cast<uint64_t*>(s_fp_dyn);
    for (uint32_t i = t; i < 2u * R; i += 256u) l[i] = tbl_g[i];
    tbl = l;
  }
  __syncthreads();
  const uint64_t nw = (uint64_t)gridDim.x * 4u;
  for (uint64_t k = (uint64_t)blockIdx.x * 4u + (t >> 6); k < npairs; k += nw) {  // no barrier below
    const uint64_t c0 = pairs[2u * k] * R;
    uint64_t acc = 0;
    for (uint32_t col = lane; col < R; col += 64u) {
      const uint32_t x = v[c0 + col];
      if (x == 0u) continue;
      uint32_t m = 0;
      if (MASKS && x == 2u) m = masks[c0 + col];
      acc += fp_cell(x, m, tbl, col, R, msg_codes);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += (uint64_t)__shfl_xor((unsigned long long)acc, off, 64);
    if (lane == 0u) {
      fp_out[k] = acc;
      flags[k] = acc != kept[pairs[2u * k + 1u]] ? 1u : 0u;
    }
  }
}
extern "C" hipError_t kpe_launch_fp_pairs(const uint8_t* v, const uint32_t* masks, uint32_t R, const uint64_t* pairs,
                                          uint64_t npairs, const uint64_t* tbl, uint32_t msg_codes, const uint64_t* kept,
                                          uint64_t* fp_out, uint8_t* flags, hipStream_t s) {
  if (!npairs) return hipSuccess;
  if (R > kFpMaxRules) return hipErrorInvalidValue;
  const dim3 grid((unsigned)std::min<uint64_t>((npairs + 3u) / 4u, kFpGrid));
  const uint32_t lds = R && R <= kFpLdsRules ? 1u : 0u;
  const size_t dyn = lds ? (size_t)R * 16u : 0u;
  if (masks)
    hipLaunchKernelGGL(kpe_fp_pairs_kernel<true>, grid, dim3(256), dyn, s, v, masks, R, pairs, npairs, tbl, lds, msg_codes,
                       kept, fp_out, flags);
  else
    hipLaunchKernelGGL(kpe_fp_pairs_kernel<false>, grid, dim3(256), dyn, s, v, masks, R, pairs, npairs, tbl, lds, msg_codes,
                       kept, fp_out, flags);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Kept results carried into a gathered corpus (kpe_results_gather): output row k is row pairs[2k + 1]
// of source pairs[2k], the sources' base pointers in a device table (gather.inl, shared with
// scripts/corpus_gather_check.cpp). One contiguous byte range of the output per block, whole words
// between its aligned ends, byte stores for the matrix's last partial word; no atomics, no zeroing pass.
#define KPE_GA_FN __host__ __device__ __forceinline__
#define KPE_GA_DEV __device__ __forceinline__
namespace {
__device__ __forceinline__ uint32_t ga_load4(const uint8_t* p) { return *reinterpret_cast<const uint32_t*>(p); }
__device__ __forceinline__ void ga_store4(uint8_t* p, uint32_t w) { *reinterpret_cast<uint32_t*>(p) = w; }
#include "gather.inl"
}  // namespace

__global__ void __launch_bounds__(256) kpe_results_gather_kernel(const uint8_t* const* __restrict__ tab,
                                                                 const uint64_t* __restrict__ pairs, uint64_t total,
                                                                 uint32_t R, uint8_t* __restrict__ out) {
  const GaRange G = ga_range(total, gridDim.x, blockIdx.x);
  ga_copy(G, threadIdx.x, tab, pairs, R, out);
}
__global__ void __launch_bounds__(256) kpe_fp_gather_pairs_kernel(const uint64_t* const* __restrict__ tab,
                                                                  const uint64_t* __restrict__ pairs, uint64_t npairs,
                                                                  uint64_t* __restrict__ out) {
  for (uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x; k < npairs; k += (uint64_t)gridDim.x * 256u)
    ga_fp(k, tab, pairs, out);
}
extern "C" hipError_t kpe_launch_results_gather(const uint8_t* const* tab, const uint64_t* pairs, uint64_t npairs,
                                                uint32_t R, uint8_t* out, hipStream_t s) {
  const uint64_t total = npairs * R;
  if (!total) return hipSuccess;
  if (((uintptr_t)out & 3u) != 0u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kpe_results_gather_kernel, dim3(ga_grid(total)), dim3(kGaLanes), 0, s, tab, pairs, total, R, out);
  return hipGetLastError();
}
extern "C" hipError_t kpe_launch_fp_gather_pairs(const uint64_t* const* tab, const uint64_t* pairs, uint64_t npairs,
                                                 uint64_t* out, hipStream_t s) {
  if (!npairs) return hipSuccess;
  const dim3 grid((unsigned)std::min<uint64_t>((npairs + 255u) / 256u, 1u << 16));
  hipLaunchKernelGGL(kpe_fp_gather_pairs_kernel, grid, dim3(256), 0, s, tab, pairs, npairs, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Report detail of a row list (kpe_fetch_report_rows): the selection chain over the compact matrix
// kpe_gather_rows_kernel made of the listed rows, for three need tables at once (report_rows.inl,
// shared with scripts/report_rows_check.cpp). The count pass writes three counts per tile, kind k at
// tile_counts[k * ntiles + tile]; kpe_select_scan_kernel scans the 3 * ntiles counts in one launch;
// the scatter pass recomputes the hit masks and writes each hit's compact cell and its payload,
// fetched through rows[]. Ordering is the selection's: tile offset + waves before (LDS) + lanes
// before (DPP scan); no global cursor, no atomics. The need tables are staged in LDS up to
// kSelLdsRules rules (48 KiB) and the slot table beside them up to kRrSlotLdsRules; past that they are
// read from global memory: no rule limit.
#define KPE_RR_FN __host__ __device__ __forceinline__
#define KPE_RR_DEV __device__ __forceinline__
namespace {
__device__ __forceinline__ void rr_load16(const uint8_t* __restrict__ p, uint32_t cnt, uint32_t* w) {
  const Cells16 c = load_cells(p, 0, cnt);
  w[0] = c.w[0], w[1] = c.w[1], w[2] = c.w[2], w[3] = c.w[3];
}
#include "report_rows.inl"
}  // namespace
constexpr uint32_t kRrSlotLdsRules = 4096;  // the slot table's 4 R bytes staged beside the need tables
static_assert(kRrTile == kSelTile, "the tiles of the selection kernels");

template <bool LDS>
__global__ void __launch_bounds__(256) kpe_report_need_count_kernel(const uint8_t* __restrict__ v, uint64_t cells, uint32_t R,
                                                                    const uint8_t* __restrict__ need_g,
                                                                    uint32_t* __restrict__ tile_counts, uint64_t ntiles) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_rr_dyn[];
  __shared__ uint32_t s_w[2][kRrKinds][4];  // by tile parity: one barrier per tile
  const uint32_t t = threadIdx.x;
  const uint8_t* need = stage_table<LDS>(need_g, 3u * R, s_rr_dyn);
  uint32_t par = 0;
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x, par ^= 1u) {
    uint32_t m[kRrKinds];
    rr_lane_hits(v, cells, R, tile, t, need, m);
#pragma unroll
    for (uint32_t k = 0; k < kRrKinds; ++k) {
      const uint32_t inc = wave_incl_scan((uint32_t)__popc(m[k]));
      if ((t & 63u) == 63u) s_w[par][k][t >> 6] = inc;
    }
    __syncthreads();
    if (t < kRrKinds) tile_counts[t * ntiles + tile] = s_w[par][t][0] + s_w[par][t][1] + s_w[par][t][2] + s_w[par][t][3];
  }
}

template <bool LDS>
__global__ void __launch_bounds__(256) kpe_report_need_scatter_kernel(const uint8_t* __restrict__ v, uint64_t cells,
                                                                      uint32_t R, const uint8_t* __restrict__ need_g,
                                                                      uint32_t slot_lds, const uint64_t* __restrict__ offs,
                                                                      uint64_t ntiles, KpeRrSrc S, const KpeRrOut O) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_rr_dyn[];
  __shared__ uint32_t s_w[kRrKinds][4];
  const uint32_t t = threadIdx.x;
  if (LDS && slot_lds) {  // uniform; behind the need tables, word aligned; stage_table's barrier covers it
    uint32_t* l = reinterpret_cast<uint32_t*>(s_rr_dyn + ((3u * R + 3u) & ~3u));
    for (uint32_t i = t; i < R; i += 256u) l[i] = S.slot[i];
    S.slot = l;
  }
  const uint8_t* need = stage_table<LDS>(need_g, 3u * R, s_rr_dyn);
  uint64_t base[kRrKinds];
#pragma unroll
  for (uint32_t k = 0; k < kRrKinds; ++k) base[k] = offs[k * ntiles];
  for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    uint64_t o0[kRrKinds], o1[kRrKinds];  // uniform
#pragma unroll
    for (uint32_t k = 0; k < kRrKinds; ++k) {
      o0[k] = offs[k * ntiles + tile] - base[k];
      o1[k] = offs[k * ntiles + tile + 1u] - base[k];
    }
    if (!rr_tile_live(o0, o1, O)) continue;
    uint32_t m[kRrKinds], before[kRrKinds];
    rr_lane_hits(v, cells, R, tile, t, need, m);
#pragma unroll
    for (uint32_t k = 0; k < kRrKinds; ++k) {
      const uint32_t hits = (uint32_t)__popc(m[k]);
      const uint32_t inc = wave_incl_scan(hits);
      if ((t & 63u) == 63u) s_w[k][t >> 6] = inc;
      before[k] = inc - hits;
    }
    __syncthreads();
    uint64_t o[kRrKinds];
#pragma unroll
    for (uint32_t k = 0; k < kRrKinds; ++k) {
#pragma unroll
      for (uint32_t w = 0; w < 3u; ++w)
        if (w < (t >> 6)) before[k] += s_w[k][w];
      o[k] = o0[k] + before[k];
    }
    rr_lane_scatter(rr_lane_first(tile, t), m, o, R, S, O);
    __syncthreads();
  }
}

// One thread per listed cell: the four condition trace words of a validate.foreach cell, for the
// pattern trace jobs of kpe_pattern_traces and kpe_fetch_report_rows (zeros for other rules).
__global__ void __launch_bounds__(256) kpe_fe_words_gather_kernel(const uint64_t* __restrict__ cells, uint64_t n, uint32_t R,
                                                                  const uint32_t* __restrict__ slot,
                                                                  const uint32_t* __restrict__ mtrace, uint32_t nmsg,
                                                                  uint4* __restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
    const uint64_t cell = cells[i];
    const uint64_t row = rr_div(cell, R);
    const uint32_t e = slot[(uint32_t)(cell - row * R)];
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    if (KPE_RR_SLOT_WIDTH(e) == KPE_FE_TRACE_WORDS) {
      const uint32_t* src = mtrace + row * nmsg + KPE_RR_SLOT_FIRST(e);
      w = make_uint4(src[0], src[1], src[2], src[3]);
    }
    out[i] = w;
  }
}

extern "C" uint64_t kpe_report_need_tiles(uint64_t cells) { return (cells + kRrTile - 1u) / kRrTile; }
extern "C" hipError_t kpe_launch_report_need_count(const uint8_t* v, uint64_t cells, uint32_t R, const uint8_t* need,
                                                   uint32_t* tile_counts, uint64_t* tile_offs, hipStream_t s) {
  if (!cells || !R) return hipSuccess;
  const uint64_t ntiles = kpe_report_need_tiles(cells);
  const dim3 grid((unsigned)std::min<uint64_t>(ntiles, kSelGrid));
  if (R <= kSelLdsRules)
    hipLaunchKernelGGL(kpe_report_need_count_kernel<true>, grid, dim3(256), (size_t)3u * R, s, v, cells, R, need,
                       tile_counts, ntiles);
  else
    hipLaunchKernelGGL(kpe_report_need_count_kernel<false>, grid, dim3(256), 0, s, v, cells, R, need, tile_counts, ntiles);
  hipLaunchKernelGGL(kpe_select_scan_kernel, dim3(1), dim3(256), 0, s, tile_counts, tile_offs, kRrKinds * ntiles);
  return hipGetLastError();
}
extern "C" hipError_t kpe_launch_report_need_scatter(const uint8_t* v, uint64_t cells, uint32_t R, const uint8_t* need,
                                                     const uint64_t* tile_offs, const KpeRrSrc* src, const KpeRrOut* out,
                                                     hipStream_t s) {
  if (!cells || !R || !(out->mask_cap | out->cond_cap | out->pattern_cap)) return hipSuccess;
  const uint64_t ntiles = kpe_report_need_tiles(cells);
  const dim3 grid((unsigned)std::min<uint64_t>(ntiles, kSelGrid));
  const uint32_t slot_lds = R <= kRrSlotLdsRules ? 1u : 0u;
  const size_t dyn = (((size_t)3u * R + 3u) & ~(size_t)3u) + (slot_lds ? (size_t)4u * R : 0u);
  if (R <= kSelLdsRules)
    hipLaunchKernelGGL(kpe_report_need_scatter_kernel<true>, grid, dim3(256), dyn, s, v, cells, R, need, slot_lds,
                       tile_offs, ntiles, *src, *out);
  else
    hipLaunchKernelGGL(kpe_report_need_scatter_kernel<false>, grid, dim3(256), 0, s, v, cells, R, need, 0u, tile_offs,
                       ntiles, *src, *out);
  return hipGetLastError();
}
extern "C" hipError_t kpe_launch_fe_words_gather(const uint64_t* cells, uint64_t n, uint32_t R, const uint32_t* slot,
                                                 const uint32_t* mtrace, uint32_t nmsg, uint32_t* out, hipStream_t s) {
  if (!n) return hipSuccess;
  const dim3 grid((unsigned)std::min<uint64_t>((n + 255u) / 256u, 1u << 16));
  hipLaunchKernelGGL(kpe_fe_words_gather_kernel, grid, dim3(256), 0, s, cells, n, R, slot, mtrace, nmsg,
                     reinterpret_cast<uint4*>(out));
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Per-namespace rule counts (kpe_fetch_namespace_counts): the verdict matrix grouped by the row's
// namespace, 6 uint32 counters per (namespace, rule): pass, fail, warn, error, skip, undecided (raw
// verdict codes; KPE_NA and codes outside the alphabet are not counted). The inverted-index form:
// the host sorts the row ids by namespace once per corpus (`rows`) and cuts each namespace into
// work items of at most kNsChunk rows (KpeNsItem). A block takes one item at a time, so every
// contribution it sums has the same namespace, and counts in registers: a counter is a 10-bit
// field of a 64-bit word (an item has at most 1023 rows, so no field overflows, in a lane or in a
// sum over the block). Memory sees at most one add per (namespace, rule, counter) per item, and
// only for non-zero counters: a plain store when the namespace is one item (the window is zeroed
// before the launch), an integer atomic add otherwise. Integer adds only: the table is exact and
// does not depend on the schedule.
constexpr uint32_t kNsChunk = 512;    // rows per work item (<= 1023: the 10-bit fields)
constexpr uint32_t kNsGrid = 2048;    // persistent blocks (8 per CU)
constexpr uint32_t kNsNarrow = 16;    // R below this: one row per lane (kpe_ns_count_narrow_kernel)
constexpr uint32_t kNsLdsUnits = 128; // column units a block sums in LDS (wider tiles: one lane per unit, no LDS)
constexpr uint32_t kNsBatch = 8;      // row loads a lane keeps in flight
static_assert(kNsChunk <= 1023u, "10-bit counters");

namespace {
// verdict code -> its 10-bit field of the packed counters (0 for codes that are not counted).
// Code -> field: PASS 0, FAIL 1, WARN 2, ERROR 3, SKIP 4, UNDECIDED (7) 5
__device__ __forceinline__ uint64_t ns_inc(uint32_t x) {
  const uint32_t f = x < 8u ? (0x5F43210Fu >> (4u * x)) & 15u : 15u;
  return f < 6u ? (uint64_t)1 << (10u * f) : (uint64_t)0;
}
__device__ __forceinline__ void ns_emit(uint32_t* __restrict__ o, uint32_t c, bool single) {
  if (!c) return;
  if (single) *o = c;
  else atomicAdd(o, c);
}
}  // namespace

// R >= kNsNarrow. The row is cut into units of VEC columns (VEC = 4 when R is a multiple of 4: a
// unit is one aligned 32-bit load, and a word of four KPE_NA cells is passed over; VEC = 1
// otherwise) and the units into tiles of W = min(units, 256). Thread t owns unit t % W of the tile
// and the item's rows t / W, t / W + 256 / W, ...: lanes of a wave lie along the row (coalesced
// loads, different counters). With one slice (W > 128) a lane's counters are final and go to memory
// from registers; otherwise the slices are summed in LDS first (a lane's at most 6 * VEC non-zero
// counters, different words for different lanes of a slice).
template <uint32_t VEC>
__global__ void __launch_bounds__(256) kpe_ns_count_kernel(const uint8_t* __restrict__ v, uint32_t R,
                                                           const uint32_t* __restrict__ rows,
                                                           const KpeNsItem* __restrict__ items, uint32_t nitems,
                                                           uint32_t g0, uint32_t* __restrict__ out) {
  __shared__ uint32_t s_cnt[kNsLdsUnits * 4u * 6u];
  const uint32_t t = threadIdx.x;
  const uint32_t units = R / VEC;  // VEC divides R
  const uint32_t W = units < 256u ? units : 256u;
  const uint32_t slices = 256u / W;
  const uint32_t u = t % W, sl = t / W;
  const bool lds = slices > 1u;  // then W <= kNsLdsUnits
  if (lds) {
    for (uint32_t i = t; i < W * VEC * 6u; i += 256u) s_cnt[i] = 0u;
    __syncthreads();
  }
  for (uint32_t it = blockIdx.x; it < nitems; it += gridDim.x) {
    const KpeNsItem item = items[it];
    uint32_t* __restrict__ o = out + (size_t)(item.g - g0) * R * 6u;
    const bool single = item.single != 0u;
    for (uint32_t u0 = 0; u0 < units; u0 += W) {
      const uint32_t uu = u0 + u;
      const bool on = sl < slices && uu < units;
      uint64_t acc[VEC];
#pragma unroll
      for (uint32_t j = 0; j < VEC; ++j) acc[j] = 0;
      if (on) {
        const uint8_t* __restrict__ base = v + (size_t)uu * VEC;
        // the unit of one row: a 32-bit word of four cells, or one cell
        auto load = [&](uint32_t row) -> uint32_t {
          const uint8_t* p = base + (size_t)row * R;
          return VEC == 4u ? *reinterpret_cast<const uint32_t*>(p) : (uint32_t)p[0];
        };
        auto count = [&](uint32_t w) {
          if (w == 0u) return;  // KPE_NA cells (a word of four of them): nothing to count
#pragma unroll
          for (uint32_t j = 0; j < VEC; ++j) acc[j] += ns_inc((w >> (8u * j)) & 0xFFu);
        };
        // kNsBatch rows' loads are issued before the first is counted (the rows are a gather)
        uint32_t i = item.begin + sl;
        for (; i + (kNsBatch - 1u) * slices < item.end; i += kNsBatch * slices) {
          uint32_t w[kNsBatch];
#pragma unroll
          for (uint32_t b = 0; b < kNsBatch; ++b) w[b] = load(rows[i + b * slices]);
#pragma unroll
          for (uint32_t b = 0; b < kNsBatch; ++b) count(w[b]);
        }
        for (; i < item.end; i += slices) count(load(rows[i]));
      }
      if (!lds) {
        if (on) {
#pragma unroll
          for (uint32_t j = 0; j < VEC; ++j)
#pragma unroll
            for (uint32_t k = 0; k < 6u; ++k)
              ns_emit(o + ((size_t)uu * VEC + j) * 6u + k, (uint32_t)(acc[j] >> (10u * k)) & 1023u, single);
        }
        continue;
      }
      if (on) {
#pragma unroll
        for (uint32_t j = 0; j < VEC; ++j)
#pragma unroll
          for (uint32_t k = 0; k < 6u; ++k) {
            const uint32_t c = (uint32_t)(acc[j] >> (10u * k)) & 1023u;
            if (c) atomicAdd(&s_cnt[(u * VEC + j) * 6u + k], c);
          }
      }
      __syncthreads();
      const uint32_t wn = (units - u0 < W ? units - u0 : W) * VEC * 6u;  // this tile's counters
      for (uint32_t i = t; i < wn; i += 256u) {
        const uint32_t c = s_cnt[i];
        if (c) {
          s_cnt[i] = 0u;
          ns_emit(o + (size_t)u0 * VEC * 6u + i, c, single);
        }
      }
      __syncthreads();
    }
  }
}

// R < kNsNarrow (the C2 shape, R = 3): one row per lane, the row's R bytes, one packed register
// per column. The columns' registers are summed over the wave with shuffles and over the four
// waves through LDS (4 x R words): no atomics on a few hot LDS words.
__global__ void __launch_bounds__(256) kpe_ns_count_narrow_kernel(const uint8_t* __restrict__ v, uint32_t R,
                                                                  const uint32_t* __restrict__ rows,
                                                                  const KpeNsItem* __restrict__ items, uint32_t nitems,
                                                                  uint32_t g0, uint32_t* __restrict__ out) {
  __shared__ uint64_t s_part[4][kNsNarrow];
  const uint32_t t = threadIdx.x;
  for (uint32_t it = blockIdx.x; it < nitems; it += gridDim.x) {
    const KpeNsItem item = items[it];
    uint64_t acc[kNsNarrow - 1u];
#pragma unroll
    for (uint32_t c = 0; c < kNsNarrow - 1u; ++c) acc[c] = 0;
    for (uint32_t i = item.begin + t; i < item.end; i += 256u) {
      const uint8_t* __restrict__ p = v + (size_t)rows[i] * R;
#pragma unroll
      for (uint32_t c = 0; c < kNsNarrow - 1u; ++c)
        if (c < R) acc[c] += ns_inc(p[c]);
    }
#pragma unroll
    for (uint32_t c = 0; c < kNsNarrow - 1u; ++c) {
      if (c < R) {  // uniform
        uint64_t a = acc[c];
#pragma unroll
        for (uint32_t d = 32u; d; d >>= 1) {
          const uint32_t lo = __shfl_xor((int)(uint32_t)a, (int)d, 64), hi = __shfl_xor((int)(uint32_t)(a >> 32), (int)d, 64);
          a += (uint64_t)lo | ((uint64_t)hi << 32);
        }
        if ((t & 63u) == 0u) s_part[t >> 6][c] = a;
      }
    }
    __syncthreads();
    if (t < R * 6u) {
      const uint32_t c = t / 6u, k = t - c * 6u;
      const uint64_t a = s_part[0][c] + s_part[1][c] + s_part[2][c] + s_part[3][c];
      ns_emit(out + (size_t)(item.g - g0) * R * 6u + t, (uint32_t)(a >> (10u * k)) & 1023u, item.single != 0u);
    }
    __syncthreads();
  }
}

// items: the work items of groups [g0, g0 + ng) (every item.g lies in it, every rows[] entry of
// [begin, end) is a row of the matrix); out: ng x R x 6 words, zeroed by the caller on s.
extern "C" hipError_t kpe_launch_ns_counts(const uint8_t* v, uint32_t R, const uint32_t* rows, const KpeNsItem* items,
                                           uint64_t nitems, uint32_t g0, uint32_t* out, hipStream_t s) {
  if (!nitems || !R) return hipSuccess;
  if (nitems > 0xFFFFFFFFull) return hipErrorInvalidValue;
  const dim3 grid((unsigned)std::min<uint64_t>(nitems, kNsGrid));
  if (R < kNsNarrow)
    hipLaunchKernelGGL(kpe_ns_count_narrow_kernel, grid, dim3(256), 0, s, v, R, rows, items, (uint32_t)nitems, g0, out);
  else if (R % 4u == 0u)
    hipLaunchKernelGGL(kpe_ns_count_kernel<4u>, grid, dim3(256), 0, s, v, R, rows, items, (uint32_t)nitems, g0, out);
  else
    hipLaunchKernelGGL(kpe_ns_count_kernel<1u>, grid, dim3(256), 0, s, v, R, rows, items, (uint32_t)nitems, g0, out);
  return hipGetLastError();
}
extern "C" uint32_t kpe_ns_chunk_rows(void) { return kNsChunk; }
