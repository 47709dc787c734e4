// The condition kernel's plain instance (no pattern VM) and the launcher of every instance.
#include "kernels_common.h"

#include "cond_kernel.inl"

extern "C" hipError_t kpe_launch_cond(const CondArgs* dargs, int64_t n, int fepat, int filt, int txt, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (filt) return kpe_launch_cond_filt(dargs, n, txt, s);
  if (fepat) return kpe_launch_cond_fepat(dargs, n, txt, s);
  const size_t lds = txt ? 128u * 2u * KPE_TXT_CAP : 0u;
  hipLaunchKernelGGL(kpe_cond_kernel<false>, dim3((unsigned)((n + 127) / 128)), dim3(128), lds, s, dargs);
  return hipGetLastError();
}
