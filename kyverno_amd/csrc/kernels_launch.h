// The host/device launch interface: every extern "C" launcher and query that the kernel sources
// (*.hip) define and kpe_api.cpp calls, declared once. Both sides include this header, so a
// launcher whose parameters differ from its declaration fails to compile where it is defined.
// (The argument structs stay in kernels_abi.h, which is free of HIP types.)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "kernels_abi.h"

// Scan-kernel selection: the `kind` argument of kpe_scan_grid / kpe_launch_scan / kpe_launch_prep,
// Binding::lean_kind / gen_code and kpe_kernel_stats::scan_kernel (include/kpe.h). The numbers are
// public (kpe_debug_lean_kind, bench.py, the tests) and do not change.
enum KpeScanKind : int {
  KPE_SCAN_WIDE = 0,     // kpe_scan_kernel, transposed rule pass
  KPE_SCAN_NARROW = 1,   // kpe_scan_kernel, per-lane rule loop
  KPE_SCAN_LEAN = 2,     // kpe_scan_kernel<PSS, NARROW, LEAN>: the LEAN template instance
  KPE_SCAN_PSUM = 4,     // flag on WIDE / NARROW: PSS tiles read the scan records, no lists
  KPE_SCAN_LEAN6 = 7,    // kpe_lean6_kernel (kpe_launch_lean6; sizes its own grid)
  KPE_SCAN_BATCHED = 9,  // kpe_kernel_stats::scan_kernel only: LEAN6 over several bound shards
};

extern "C" {
// scan.hip
hipError_t kpe_launch_pred(const PredArgs* a, uint32_t xblocks, hipStream_t s);
uint32_t kpe_scan_grid(int64_t n, int pss, int kind, size_t dyn_bytes);
hipError_t kpe_launch_scan(const ScanArgs* dargs, int64_t n, int pss, int kind, uint32_t grid, size_t dyn_bytes,
                           hipStream_t s);
hipError_t kpe_launch_prep(const ScanArgs* dargs, int pss, int narrow, size_t dyn_bytes, hipStream_t s);
hipError_t kpe_launch_selmask(const SelMaskArgs* a, hipStream_t s);
// cp: 0 the wide records, 1 the compact columns (gather form), 2 the owner-tagged columns (scatter form),
// 3 the same with the pod word column in LeanShard::rec12 (narrow form; tpw 2 or 4), 4 the narrow form's
// group form (tpw 4; LeanBatchArgs::wave_words sized for it)
hipError_t kpe_launch_lean6(const LeanBatchArgs* a, size_t dyn_bytes, int lc, int sann, int cv, int cp, hipStream_t s);
int kpe_lean6_compact(int lc, int cv);  // may a launch of that shape read the compact columns (cp)?
hipError_t kpe_launch_lean_pack(const LeanPackArgs* a, hipStream_t s);
hipError_t kpe_launch_lean_tag(const LeanTagArgs* a, hipStream_t s);
hipError_t kpe_launch_psa_codes(const PsaCodeArgs* a, hipStream_t s);
hipError_t kpe_launch_psum(const PsumArgs* a, hipStream_t s);
// pattern.hip, pattern_trace.hip
hipError_t kpe_launch_leaf_table(const PatArgs* dargs, const uint32_t* slot_leaf, uint32_t nslots, uint64_t nscal,
                                 hipStream_t s);
hipError_t kpe_launch_pattern(const PatArgs* dargs, int64_t n, uint32_t npr, int lt, hipStream_t s);
hipError_t kpe_launch_pattern_trace(const PatArgs* dargs, const uint64_t* cells, uint64_t n, uint32_t* out,
                                    const uint4* jobs, hipStream_t s);
// cond.hip, cond_fepat.hip, cond_filt.hip (kpe_launch_cond forwards to the other two launchers)
// (filt: the program holds a filter step `[?P]`: cond_filt.hip's build of the kernel)
hipError_t kpe_launch_cond(const CondArgs* dargs, int64_t n, int fepat, int filt, int txt, hipStream_t s);
hipError_t kpe_launch_cond_filt(const CondArgs* dargs, int64_t n, int txt, hipStream_t s);
hipError_t kpe_launch_cond_fepat(const CondArgs* dargs, int64_t n, int txt, hipStream_t s);
// pssx.hip
hipError_t kpe_launch_pssx(const PssxArgs* dargs, int64_t n, hipStream_t s);
// results.hip
hipError_t kpe_launch_count(const uint8_t* verdicts, int64_t n, uint32_t R, unsigned long long* out, hipStream_t s);
hipError_t kpe_launch_fill_rows(uint8_t* verdicts, uint32_t R, const uint32_t* rows, uint32_t nrows, uint8_t value,
                                hipStream_t s);
hipError_t kpe_launch_apply_one(uint8_t* verdicts, uint32_t* masks, int64_t n, uint32_t R, const uint32_t* segs,
                                uint32_t nsegs, hipStream_t s);
// retired rows (kpe_corpus_retire_rows): the listed rows' R verdict bytes to KPE_NA and, when masks is
// not NULL, their R mask words to 0. verdicts is 4-byte aligned; rows < N, any order.
hipError_t kpe_launch_retire_rows(uint8_t* verdicts, uint32_t* masks, uint32_t R, const uint32_t* rows, uint32_t nrows,
                                  hipStream_t s);
hipError_t kpe_launch_pack3(const uint8_t* v, uint64_t cells, uint32_t* out, hipStream_t s);
hipError_t kpe_launch_select_count(const uint8_t* v, uint64_t cells, uint32_t R, const uint8_t* sel, int na_selected,
                                   uint32_t* tile_counts, uint64_t* tile_offs, hipStream_t s);
hipError_t kpe_launch_select_scatter(const uint8_t* v, uint64_t cells, uint32_t R, const uint8_t* sel, int na_selected,
                                     const uint64_t* tile_offs, uint64_t cap, uint64_t* out_cells, uint8_t* out_v,
                                     hipStream_t s);
hipError_t kpe_launch_row_summary(const uint8_t* v, uint32_t R, uint64_t row0, uint64_t nrows, const uint8_t* unscored,
                                  uint32_t* out, hipStream_t s);
hipError_t kpe_launch_ns_counts(const uint8_t* v, uint32_t R, const uint32_t* rows, const KpeNsItem* items,
                                uint64_t nitems, uint32_t g0, uint32_t* out, hipStream_t s);
uint32_t kpe_ns_chunk_rows(void);
// result deltas (kpe_changed_rows, kpe_delta_transitions). tab: Rn words, the kept column of new
// column r in bits 0-15 (0xFFFF: none) and its `always` mask in bits 16-23; unmapped: Ro bytes,
// non-zero for a kept column no new column names (NULL: there is none); flags: n bytes, one per
// row, each written once. Rn, Ro <= kpe_delta_max_rules().
hipError_t kpe_launch_delta_flags(const uint8_t* vnew, const uint8_t* vold, uint64_t n, uint32_t Rn, uint32_t Ro,
                                  const uint32_t* tab, const uint8_t* unmapped, uint8_t* flags, hipStream_t s);
// out: nrows x R bytes, row i = row rows[i] of v
hipError_t kpe_launch_gather_rows(const uint8_t* v, uint32_t R, const uint64_t* rows, uint64_t nrows, uint8_t* out,
                                  hipStream_t s);
// out: Rn x 64 counters (old code x 8 + new code), zeroed here
hipError_t kpe_launch_delta_transitions(const uint8_t* vnew, const uint8_t* vold, uint64_t n, uint32_t Rn, uint32_t Ro,
                                        const uint32_t* tab, unsigned long long* out, hipStream_t s);
uint32_t kpe_delta_max_rules(void);
// policy edits on a kept result (kpe_results_splice): out (n x rn) from kept (n x Ro) and sub (n x Rs).
// col: 2 rn words, per output column {source column | 0x80000000 for a column of sub, partner kept
// column in bits 0-15 (0xFFFF: none) | `always` mask in bits 16-23} (the second word counts for
// columns of sub only); unmapped: Ro bytes, non-zero for a kept column that is neither copied nor a
// partner (NULL: there is none); flags: n bytes, one per row, each written once. out is 16-byte
// aligned and overlaps neither input. Ro, Rs, rn <= kpe_delta_max_rules().
hipError_t kpe_launch_splice(const uint8_t* kept, const uint8_t* sub, uint64_t n, uint32_t Ro, uint32_t Rs, uint32_t rn,
                             const uint32_t* col, const uint8_t* unmapped, uint8_t* out, uint8_t* flags, hipStream_t s);
uint32_t kpe_splice_rows_per_group(uint32_t Ro, uint32_t Rs, uint32_t rn);  // rows of a group of that pass
uint32_t kpe_splice_grid(void);                                             // its most blocks
// result deltas across corpora (kpe_changed_pairs). pairs: npairs x {row of vnew, row of vold};
// tab / unmapped as above; flags: npairs bytes, one per pair, each written once.
hipError_t kpe_launch_delta_pairs(const uint8_t* vnew, const uint8_t* vold, const uint64_t* pairs, uint64_t npairs,
                                  uint32_t Rn, uint32_t Ro, const uint32_t* tab, const uint8_t* unmapped, uint8_t* flags,
                                  hipStream_t s);
// out[i] = pairs[2 * idx[i]] (the new row of pair idx[i]), m words
hipError_t kpe_launch_pair_rows(const uint64_t* pairs, const uint64_t* idx, uint64_t m, uint64_t* out, hipStream_t s);

// row fingerprints (kpe_fetch_row_fingerprints, kpe_fingerprints_keep, kpe_changed_rows_fp). tbl:
// 2 R words, [salts][msg_salts]; masks: the N x R cv mask words, or NULL when they do not count;
// out: nrows words, row row0 + i at out[i], each written once. 1 <= R <= kpe_delta_max_rules().
hipError_t kpe_launch_row_fp(const uint8_t* v, const uint32_t* masks, uint32_t R, uint64_t row0, uint64_t nrows,
                             const uint64_t* tbl, uint32_t msg_codes, uint64_t* out, hipStream_t s);
// flags[i] = a[i] != b[i], n bytes
hipError_t kpe_launch_fp_diff(const uint64_t* a, const uint64_t* b, uint64_t n, uint8_t* flags, hipStream_t s);
// out[i] = fp[rows[i]], m words
hipError_t kpe_launch_fp_gather(const uint64_t* fp, const uint64_t* rows, uint64_t m, uint64_t* out, hipStream_t s);
// the fingerprint form over a pair list (kpe_changed_pairs_fp): fp_out[k] = the fingerprint of row
// pairs[2 k] of v, flags[k] = it differs from kept[pairs[2 k + 1]]. R <= kpe_delta_max_rules() (0 allowed).
hipError_t kpe_launch_fp_pairs(const uint8_t* v, const uint32_t* masks, uint32_t R, const uint64_t* pairs, uint64_t npairs,
                               const uint64_t* tbl, uint32_t msg_codes, const uint64_t* kept, uint64_t* fp_out,
                               uint8_t* flags, hipStream_t s);

// kept results gathered across corpora (kpe_results_gather). tab: the sources' base pointers, in
// device memory; pairs: npairs x {source, row}, in device memory, every pair inside its source. out:
// npairs x R bytes (4-byte aligned) / npairs words, row k = row pairs[2k + 1] of tab[pairs[2k]],
// each byte written once. out overlaps no source.
hipError_t kpe_launch_results_gather(const uint8_t* const* tab, const uint64_t* pairs, uint64_t npairs, uint32_t R,
                                     uint8_t* out, hipStream_t s);
hipError_t kpe_launch_fp_gather_pairs(const uint64_t* const* tab, const uint64_t* pairs, uint64_t npairs, uint64_t* out,
                                      hipStream_t s);

// report detail of a row list (kpe_fetch_report_rows) over the compact matrix v of `cells` cells
// (a multiple of R). need: 3 R bytes, [mask][cond][pattern] in the KPE_SEL convention, bit 0
// (KPE_NA) clear in every byte. tile_counts: 3 * ntiles words (+ padding to a multiple of four),
// tile_offs: 3 * ntiles + 1 offsets, ntiles = kpe_report_need_tiles(cells); kind k's hits are
// tile_offs[(k + 1) * ntiles] - tile_offs[k * ntiles]. The count launcher also runs the scan.
uint64_t kpe_report_need_tiles(uint64_t cells);
hipError_t kpe_launch_report_need_count(const uint8_t* v, uint64_t cells, uint32_t R, const uint8_t* need,
                                        uint32_t* tile_counts, uint64_t* tile_offs, hipStream_t s);
hipError_t kpe_launch_report_need_scatter(const uint8_t* v, uint64_t cells, uint32_t R, const uint8_t* need,
                                          const uint64_t* tile_offs, const KpeRrSrc* src, const KpeRrOut* out,
                                          hipStream_t s);
// out[i * KPE_FE_TRACE_WORDS + w]: the condition trace words of cell cells[i] (row * R + column) when
// its rule is a validate.foreach rule with a slot, zeros otherwise (slot: KPE_RR_SLOT per rule)
hipError_t kpe_launch_fe_words_gather(const uint64_t* cells, uint64_t n, uint32_t R, const uint32_t* slot,
                                      const uint32_t* mtrace, uint32_t nmsg, uint32_t* out, hipStream_t s);

// relabel.hip
// kpe_corpus_set_namespace_labels: r_nsl[i] = map[min(r_nsa[i], G)] for the n rows; map has G + 1
// entries (namespace id -> row of the new label table), map[G] = KPE_NO_STR
hipError_t kpe_launch_nsl_remap(const uint32_t* r_nsa, const uint32_t* map, uint32_t G, uint64_t n, uint32_t* r_nsl,
                                hipStream_t s);
}
