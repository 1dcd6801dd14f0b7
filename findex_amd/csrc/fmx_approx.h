// fmx_approx.h -- what the depth-first searches (fmx_approx.hip: substitutions; fmx_edit.hip: edit distance,
// §19) share on the device: the wave-level ordering of frame accesses and the append to the staging area.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fmx {

// writes and reads of the wave's frame by different lanes
__device__ __forceinline__ void ap_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Appends the hits of the lanes with `flag` (called by the whole wave).
__device__ __forceinline__ void ap_emit(bool flag, uint64_t q, uint32_t d, uint64_t sp, uint64_t ep, uint32_t lane,
                                        unsigned long long *__restrict__ stage, uint64_t cap,
                                        unsigned long long *__restrict__ total) {
  const unsigned long long m = __builtin_amdgcn_ballot_w64(flag);
  if (!m) return;
  unsigned long long base = 0;
  if (lane == 0) base = atomicAdd(total, (unsigned long long)__popcll(m));
  base = __shfl(base, 0, 64);
  if (flag) {
    const uint64_t pos = base + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
    if (pos < cap) {
      stage[3 * pos] = (unsigned long long)(uint32_t)q | ((unsigned long long)d << 32);
      stage[3 * pos + 1] = sp;
      stage[3 * pos + 2] = ep;
    }
  }
}

}  // namespace fmx
