// What the kernel sources (*.hip: one per kernel family, each compiled once for gfx950) share:
// the argument structs, the launcher declarations they define against, the string predicates
// and two device helpers. Everything else lives with the kernels that use it.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <stdint.h>

#include <algorithm>

#include "kernels_abi.h"
#include "kernels_launch.h"
#include "schema.h"

namespace {
#include "strmatch.inl"

// Wave-uniform table read: the address is uniform, so this is a scalar (SMEM) load
// through the constant cache — no LDS round trip and no readfirstlane to branch on it.
template <class T>
__device__ __forceinline__ T sld(const T* p, uint32_t i) {
  static_assert(sizeof(T) % 4 == 0, "word-sized tables");
  typedef __attribute__((address_space(4))) const uint32_t* cptr;
  const cptr src = (cptr)(p + i);
  T out;
  uint32_t* d = reinterpret_cast<uint32_t*>(&out);
#pragma unroll
  for (uint32_t k = 0; k < sizeof(T) / 4; ++k) d[k] = src[k];
  return out;
}

// Inclusive wave64 prefix sum: 4 row_shr steps inside each 16-lane row, then
// row_bcast:15 / row_bcast:31 across rows (6 DPP adds, no LDS).
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {
  x += __builtin_amdgcn_update_dpp(0u, x, 0x111, 0xf, 0xf, false);
  x += __builtin_amdgcn_update_dpp(0u, x, 0x112, 0xf, 0xf, false);
  x += __builtin_amdgcn_update_dpp(0u, x, 0x114, 0xf, 0xf, false);
  x += __builtin_amdgcn_update_dpp(0u, x, 0x118, 0xf, 0xf, false);
  x += __builtin_amdgcn_update_dpp(0u, x, 0x142, 0xa, 0xf, false);
  x += __builtin_amdgcn_update_dpp(0u, x, 0x143, 0xc, 0xf, false);
  return x;
}

}  // namespace
