// Failing paths of listed pattern cells (kpe_pattern_traces): one lane per cell (row * R + col)
// walks each root of the cell's rule (at most KPE_TRACE_ROOTS) from the tape in HBM with the
// VM's TRACE instance, which records the path of the last failure (PatternError.Path). A cell
// with a job (jobs[i].w != 0: a validate.foreach cell that a pattern entry decided) walks the
// entry's roots [x, x + y & 0xFFFF) (PR_* flags in y >> 16) from the element node z (kNoNode: the
// resource root) instead. Report time only; the evaluation kernels never carry the tracing code
// (an object of its own, so the TRACE instance does not lengthen the pattern compile).
#include "kernels_common.h"

namespace {
#include "patvm.inl"
}  // namespace

__global__ void __launch_bounds__(128) kpe_pattern_trace_kernel(const PatArgs* __restrict__ ap,
                                                                 const uint64_t* __restrict__ cells, uint64_t n,
                                                                 uint32_t* __restrict__ out,
                                                                 const uint4* __restrict__ jobs) {
  const uint64_t i = (uint64_t)blockIdx.x * 128u + threadIdx.x;
  if (i >= n) return;
  const PatArgs& a = *ap;
  uint32_t* rec = out + i * (KPE_TRACE_ROOTS * KPE_TRACE_WORDS);
  for (uint32_t k = 0; k < KPE_TRACE_ROOTS * KPE_TRACE_WORDS; ++k) rec[k] = 0u;
  const uint64_t cell = cells[i];
  const uint64_t row = cell / a.R;
  const uint32_t col = (uint32_t)(cell - row * a.R);
  if (row >= (uint64_t)a.n) return;
  const uint4 job = jobs ? jobs[i] : make_uint4(0u, 0u, 0u, 0u);
  KpePatRule pr;
  uint32_t start = (uint32_t)a.doc_off[row];
  if (job.w) {
    pr.r0 = job.x, pr.nr = job.y & 0xFFFFu, pr.flags = job.y >> 16;
    if (job.z != kNoNode) start = job.z;
  } else {
    if (!a.col2pr || C2P_RULE(a.col2pr[col]) == 0u) return;
    pr = a.rules[C2P_RULE(a.col2pr[col]) - 1u];
  }
  PatVM vm{a, PV_DOCVIEW(a, reinterpret_cast<const uint2*>(a.doc), 0u, a.ndoc), start,
           a.pvals + (size_t)row * a.nvars, 0u};
  if (pr.flags & PR_ANY_BAD) {
    rec[0] = KPE_TR_VALID | ((uint32_t)KPE_ERROR_ << 16);
    return;
  }
  for (uint32_t k = 0; k < pr.nr && k < KPE_TRACE_ROOTS; ++k) {
    vm.tr = rec + k * KPE_TRACE_WORDS;
    const uint32_t v = pat_match_root<true>(vm, pr.r0 + k);
    vm.tr[0] = (vm.tr[0] & 0xFFFFu) | (v << 16) | KPE_TR_VALID;
  }
}

extern "C" hipError_t kpe_launch_pattern_trace(const PatArgs* dargs, const uint64_t* cells, uint64_t n, uint32_t* out,
                                               const uint4* jobs, hipStream_t s) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(kpe_pattern_trace_kernel, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, s, dargs, cells, n, out,
                     jobs);
  return hipGetLastError();
}
