// The condition kernel built with filter steps `[?P]` (KPE_COND_FILT, condvm.inl), for programs that
// hold one (CondProgram::any_filter); kpe_launch_cond (cond.hip) forwards to it.
#define KPE_COND_FILT 1
#include "kernels_common.h"

#include "cond_kernel.inl"

extern "C" hipError_t kpe_launch_cond_filt(const CondArgs* dargs, int64_t n, int txt, hipStream_t s) {
  const size_t lds = txt ? 128u * 2u * KPE_TXT_CAP : 0u;
  hipLaunchKernelGGL(kpe_cond_filt_kernel<true>, dim3((unsigned)((n + 127) / 128)), dim3(128), lds, s, dargs);
  return hipGetLastError();
}
