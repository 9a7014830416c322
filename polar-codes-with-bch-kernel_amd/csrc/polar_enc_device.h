// polar_enc_device.h -- device code of the polar encoder's first step, shared by the
// generate / encode kernel (polar_channel.hip) and the genie-aided SC kernel
// (polar_genie.hip): one wave rebuilds u, the U encoder inputs of its word, as packed bits
// in LDS. CMixedKernelEncoder::Encode (out/external/MixedKernelEncoder.cpp:142-158): the
// information bits go to the unfrozen symbols (64 symbols per ballot), static frozen symbols
// are zeros, the dynamic constraints are walked in symbol order (a frozen symbol may depend
// on an earlier frozen one), their terms reduced across the lanes.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "polar_device.h"
#include "polar_list_device.h"

namespace bchk {
namespace penc {

using plist::wsync;

__device__ __forceinline__ uint32_t ubit(const uint32_t *u, int pos) { return (u[pos >> 5] >> (pos & 31)) & 1u; }

// information bytes in[0, K) packed: bit r of the word = bit r & 63 of ib[r >> 6]
// (wsync before another lane reads ib)
__device__ __forceinline__ void pack_info(const uint8_t *in, int K, uint64_t *ib, int lane) {
    for (int g = 0; g * 64 < K; ++g) {
        const int r = g * 64 + lane;
        const uint64_t m = __ballot(r < K && (in[r] & 1));
        if (lane == 0) ib[g] = m;
    }
}

// u into ua[(U + 63) / 64] from the packed information bits ib (visible to the wave): the
// information bits at the unfrozen symbols, zeros at the frozen ones, then the dynamic frozen
// symbols in symbol order, each the XOR of its constraint's earlier terms. ua is visible to
// the whole wave on return.
__device__ __forceinline__ void build_u(const PolarEncTables &t, const uint64_t *ib, uint64_t *ua, int lane) {
    const int U = t.U, u64s = (U + 63) / 64;
    for (int g = 0; g < u64s; ++g) {
        const int i = g * 64 + lane;
        const int r = i < U ? (int)t.inforank[i] : -1;
        const uint64_t m = __ballot(r >= 0 && ((ib[r >> 6] >> (r & 63)) & 1ull));
        if (lane == 0) ua[g] = m;
    }
    wsync();
    uint32_t *u32 = reinterpret_cast<uint32_t *>(ua);
    for (int d = 0; d < t.ndyn; ++d) {
        const uint32_t a = t.dynoff[d], e = t.dynoff[d + 1] - 1u;  // terms [a, e), the symbol at e
        uint32_t v = 0;
        for (uint32_t q = a + (uint32_t)lane; q < e; q += 64) v ^= ubit(u32, t.dynterm[q]);
        const uint32_t par = (uint32_t)__popcll(__ballot(v != 0)) & 1u;
        const int sym = t.dynterm[e];
        if (par && lane == 0) u32[sym >> 5] |= 1u << (sym & 31);
        wsync();
    }
}

}  // namespace penc
}  // namespace bchk
