// ===========================================================================
// Pattern rules: validate.MatchPattern over the document tape
// (pkg/engine/validate/validate.go:15-261, anchor/handlers.go:31-275, pattern/pattern.go).
// One lane per resource runs the compiled pattern (program.cpp pc::PatCompiler) against
// its document nodes; cells the scan kernel marked KPE_PENDING_ (rule matched) are
// resolved to pass / fail / error / skip. Only the class of the error a subtree returns
// and whether its path is empty decide the verdict, so that is all a subtree reports.
// The reference's recursion is an explicit per-lane frame stack (no calls, so no spilled
// call frames and no callee register budget): a frame is a map validated member by
// member, or an array validated element by element; scalar leaves resolve in place.
// ===========================================================================
#include "kernels_common.h"

namespace {
#include "patvm.inl"
}  // namespace

// grid: 256-row blocks, one lane per row running every pattern rule
#ifndef KPE_PAT_BLOCK
#define KPE_PAT_BLOCK 128  // C5 / C3 pattern kernel (events, profiles/r03_c_ldsframes): 256 x 8 frames 20.7 / 9.2 ms,
#endif                     // 128 x 8 18.1 / 7.8, 256 x 6 17.2 / 7.0, 128 x 6 16.8 / 6.9, + 4 waves/SIMD 15.6 / 7.0
// the lane's frame stack lives in LDS (FramesLds, word-planar: conflict-free at any mix of depths)
#ifndef KPE_PAT_MINW
#define KPE_PAT_MINW 3  // the leaf-table instance takes 111 VGPRs (4 waves/SIMD, as many as the 8 LDS-bound
                        // blocks per CU hold), the one without 166; the inline map path spills at 128 (r03_e_inline)
#endif
// LT: the leaf-table instance (PatVMT LT), for programs whose leaves all have table slots.
template <bool LT>
__global__ void __launch_bounds__(KPE_PAT_BLOCK, KPE_PAT_MINW) kpe_pattern_kernel(const PatArgs* __restrict__ ap) {
  constexpr uint32_t kWaveWords = FramesLds::kWords * FramesLds::kDepth * 64u;
  __shared__ uint32_t s_fs[KPE_PAT_BLOCK / 64][kWaveWords];
  __shared__ uint8_t s_memo[KPE_PAT_MEMO][KPE_PAT_BLOCK];  // byte-planar: a lane's slot s at [s][lane]
  const int64_t i = (int64_t)blockIdx.x * KPE_PAT_BLOCK + threadIdx.x;
  if (i >= ap->n) return;
  const int64_t r = ap->perm ? (int64_t)ap->perm[i] : i;
  pat_eval_row<FramesLds, LT, true>(*ap, r, FramesLds{&s_fs[threadIdx.x >> 6][threadIdx.x & 63u]},
                                    &s_memo[0][threadIdx.x], KPE_PAT_BLOCK);
}
// The cells kpe_pattern_kernel marked KPE_DEEP_ (one lane per row; rows without marks only scan),
// on a kPatStack-deep LDS frame stack (one-wave blocks: 25 KiB of LDS each).
template <bool LT>
__global__ void __launch_bounds__(64) kpe_pattern_deep_kernel(const PatArgs* __restrict__ ap) {
  __shared__ uint32_t s_fs[FramesLdsDeep::kWords * FramesLdsDeep::kDepth * 64u];
  if (ap->deep_any && *ap->deep_any == 0u) return;  // kpe_pattern_kernel marked no cell
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= ap->n) return;
  // rows through doc_perm (grouped by kind, then tape size) like the main kernel: the rows with deep
  // cells (one kind's deeper autogen patterns) fill whole waves instead of a few lanes of each
  const int64_t r = ap->perm ? (int64_t)ap->perm[i] : i;
  pat_deep_row<LT>(*ap, r, FramesLdsDeep{&s_fs[threadIdx.x]});
}

// Leaf table of a binding (PatArgs::ltab): grid y = slot, one thread per scalar of the corpus;
// a wave's 64 results are one ballot, stored as two words (ltab_words covers whole waves).
__global__ void __launch_bounds__(256) kpe_leaf_table_kernel(const PatArgs* __restrict__ ap,
                                                             const uint32_t* __restrict__ slot_leaf) {
  const PatArgs& a = *ap;
  const uint32_t sid = blockIdx.x * 256u + threadIdx.x, slot = blockIdx.y;
  uint32_t und = 0;
  const bool r = sid < a.nscal && pat_leaf_eval(a, sid, slot_leaf[slot], nullptr, &und);
  const uint64_t m = __ballot(r);
  if ((threadIdx.x & 63u) == 0u && sid < a.nscal) {
    uint32_t* w = a.ltab + (size_t)slot * a.ltab_words + (sid >> 5);
    w[0] = (uint32_t)m;
    w[1] = (uint32_t)(m >> 32);
  }
}
extern "C" hipError_t kpe_launch_leaf_table(const PatArgs* dargs, const uint32_t* slot_leaf, uint32_t nslots,
                                            uint64_t nscal, hipStream_t s) {
  if (nslots == 0 || nscal == 0) return hipSuccess;
  hipLaunchKernelGGL(kpe_leaf_table_kernel, dim3((unsigned)((nscal + 255) / 256), nslots), dim3(256), 0, s, dargs,
                     slot_leaf);
  return hipGetLastError();
}
extern "C" hipError_t kpe_launch_pattern(const PatArgs* dargs, int64_t n, uint32_t npr, int lt, hipStream_t s) {
  if (n <= 0 || npr == 0) return hipSuccess;
  // one lane per row running every pattern rule (a rows x rules grid measured no faster on C5 and
  // slower on C3's 600 rules; it also doubled the VM code the kernel holds)
  // (two or four lanes per row, each taking every 2nd / 4th pattern cell: C5 12.3 / 19.3 ms against
  // 8.5, profiles/r04_i: the lanes of a wave then walk different rules; verdicts of a 64-column
  // chunk written back once as whole words: C5 8.6 / C3 3.66 ms against 8.5 / 3.34, more spills,
  // profiles/r04_j)
  const dim3 grid((unsigned)((n + KPE_PAT_BLOCK - 1) / KPE_PAT_BLOCK));
  const dim3 rows((unsigned)((n + 63) / 64));
  if (lt) {
    hipLaunchKernelGGL(kpe_pattern_kernel<true>, grid, dim3(KPE_PAT_BLOCK), 0, s, dargs);
    hipLaunchKernelGGL(kpe_pattern_deep_kernel<true>, rows, dim3(64), 0, s, dargs);
  } else {
    hipLaunchKernelGGL(kpe_pattern_kernel<false>, grid, dim3(KPE_PAT_BLOCK), 0, s, dargs);
    hipLaunchKernelGGL(kpe_pattern_deep_kernel<false>, rows, dim3(64), 0, s, dargs);
  }
  return hipGetLastError();
}
