// polar_tier_device.h -- the index table of the SC-list kernels whose path state does not fit
// LDS (polar_sclist_tiered.hip, polar_mixed_tiered.hip).
//
// The outer layers of every path live in the workgroup's workspace, shared between paths and
// copied on write (Tal and Vardy's lazy copy; the reference's CTVMemoryEngine /
// CListKernelEngine::UpdateIndex, TVMemoryEngine.cpp:96-142, KernelListEngine.cpp:318-367). Per
// global layer (the all-Arikan kernel) or group (the mixed one) there are L arrays, and
// idx[t * L + q] names the array of path q in tier t. The initial path names array 0 everywhere
// (tier_init), a clone copies its parent's indices (tier_clone), a kill does nothing: an array's
// reference count is the number of active paths naming it, counted when needed, never stored.
// Resolving sharing before a write stays in each kernel (own_layer, own_group: twins up to what a
// mover copies; one shared body cost both kernels throughput).
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "polar_list_device.h"

namespace bchk {
namespace ptier {

using plist::wsync;

// the initial path pid names array 0 of every tier, whatever the last codeword left
__device__ __forceinline__ void tier_init(uint8_t *idx, int split, int L, uint32_t pid, int lane) {
    if (lane < split) idx[lane * L + (int)pid] = 0;
}
// ClonePath: l1 names l's arrays
__device__ __forceinline__ void tier_clone(uint8_t *idx, int split, int L, int l, int l1, int lane) {
    if (lane < split) idx[lane * L + l1] = idx[lane * L + l];
}

}  // namespace ptier
}  // namespace bchk
