// The condition kernel's FEPAT instance (with the pattern VM); kpe_launch_cond (cond.hip) forwards to it.
#include "kernels_common.h"

#include "cond_kernel.inl"

extern "C" hipError_t kpe_launch_cond_fepat(const CondArgs* dargs, int64_t n, int txt, hipStream_t s) {
  const size_t lds = txt ? 128u * 2u * KPE_TXT_CAP : 0u;
  hipLaunchKernelGGL(kpe_cond_kernel<true>, dim3((unsigned)((n + 127) / 128)), dim3(128), lds, s, dargs);
  return hipGetLastError();
}
