// Namespace label changes on a resident corpus (kpe_corpus_set_namespace_labels):
//  kpe_nsl_remap_kernel — every row's table row from its namespace id, after the table was replaced.
// It reads no program and no verdicts; nothing of an evaluation goes through this object.
#include "kernels_common.h"

// r_nsl[i] = map[min(r_nsa[i], G)]: map is the G + 1-entry namespace id -> table row map uploaded
// with the new table, map[G] = KPE_NO_STR (a row whose namespace id is KPE_NO_STR lands there).
// One thread per row, grid-stride; r_nsa and r_nsl are read and written once, map is G + 1 words
// and stays in cache.
__global__ void __launch_bounds__(256) kpe_nsl_remap_kernel(const uint32_t* __restrict__ r_nsa,
                                                            const uint32_t* __restrict__ map, uint32_t G, uint64_t n,
                                                            uint32_t* __restrict__ r_nsl) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
    const uint32_t g = r_nsa[i];
    r_nsl[i] = map[g < G ? g : G];
  }
}

extern "C" hipError_t kpe_launch_nsl_remap(const uint32_t* r_nsa, const uint32_t* map, uint32_t G, uint64_t n,
                                           uint32_t* r_nsl, hipStream_t s) {
  if (!n) return hipSuccess;
  const dim3 grid((unsigned)std::min<uint64_t>((n + 255u) / 256u, 1u << 14));
  hipLaunchKernelGGL(kpe_nsl_remap_kernel, grid, dim3(256), 0, s, r_nsa, map, G, n, r_nsl);
  return hipGetLastError();
}
