// ===========================================================================
// Preconditions / deny / foreach-deny conditions (condvm.inl): one lane per resource resolves
// the cells of the rules whose conditions read the resource. Runs after the scan kernel (which
// marks H_COND cells pending and writes every other handler's verdict) and before the pattern
// kernel (a pattern cell whose preconditions hold stays pending).
// The kernel template; cond.hip and cond_fepat.hip each instantiate and launch one of its two
// instances (the two long compiles of the build, so they are two objects). cond_filt.hip builds
// the same text with KPE_COND_FILT (condvm.inl: filter steps `[?P]`) as kpe_cond_filt_kernel, the
// one kernel for programs that hold a filter (its FEPAT instance, which runs every program).
// ===========================================================================
#ifndef KPE_COND_FILT
#define KPE_COND_FILT 0
#endif
#if KPE_COND_FILT
#define KPE_COND_KERNEL kpe_cond_filt_kernel
#else
#define KPE_COND_KERNEL kpe_cond_kernel
#endif
namespace {
#include "patvm.inl"
#include "condvm.inl"
}  // namespace

// FEPAT: the instance that also holds the pattern VM, for programs with foreach pattern /
// anyPattern entries (the VM's frame stack and code stay out of the plain instance)
// Programs with partial-string variables (VT_TMPL) get 2 x KPE_TXT_CAP bytes of dynamic LDS per
// lane for the substituted key / value strings; the others launch without it.
// Two waves per SIMD (four 128-lane blocks per CU, what the LDS of a program with partial-string
// variables allows): the register allocator keeps each instance within 256 VGPRs.
template <bool FEPAT>
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2)))
KPE_COND_KERNEL(const CondArgs* __restrict__ ap) {
  __shared__ char nb[128][2][16];
  extern __shared__ __attribute__((aligned(16))) uint8_t ctx[];
  const int64_t i = (int64_t)blockIdx.x * 128 + threadIdx.x;
  uint8_t* tx = ap->txt ? ctx + threadIdx.x * (2u * KPE_TXT_CAP) : nullptr;
  if (i < ap->n) cond_eval_row<FEPAT>(*ap, ap->perm ? (int64_t)ap->perm[i] : i, nb[threadIdx.x], tx);
}
