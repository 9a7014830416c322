// polar_genie.hip -- genie-aided successive cancellation on gfx950: symbol φ of every word is
// decoded with the TRUE u_0..u_{φ-1} fed back, so the per-symbol error counts over many noisy
// words rank the synthetic channels of the whole code as the shipped decoder sees them (kernel
// LLRs, min-sum approximations and layer order included). The Monte-Carlo AWGN design
// (bchk_polar_design_genie, polar_design.cpp) and the per-symbol error profile of a code
// (bchk_polar_genie_run, polar_host.cpp) are built on it.
//
// polar_genie_kernel: one 64-lane wave per word, persistent over the batch, one path. The
// wave rebuilds u from the sent information bits exactly as polar_gen_kernel does
// (polar_enc_device.h), keeps it packed in LDS, then runs the decoder's phase loop over the
// mixed layout: LoadLLRs, IterativelyCalcS with the routines of polar_llr_device.h (the f/g of
// Arikan layers, coset enumeration or the trellis Viterbi of matrix layers, the f/g processors
// of the named G / A5 layers -- the code
// polar_mixed_kernel runs, so LLR_φ is its value bit for bit for a path whose earlier decisions
// were u_0..u_{φ-1}), then IterativelyUpdateC with the true u_φ. Lane φ & 63 keeps LLR_φ in a
// register; every 64 phases (and at the end) the wave stores one coalesced row segment.
//
// polar_genie_sum_kernel: the columns of those rows summed into the per-symbol counters, a lane
// per symbol over kGenieSumRows words, then one integer atomic per symbol and workgroup:
//   err[φ]  += (LLR_φ < 0 ? 1 : 0) != u_φ                (the decoder's decision rule)
//   soft[φ] += (int64) rint(c * 65536.0f), c = s clamped to [-32768, 32768],
//              s = u_φ ? -LLR_φ : LLR_φ                   (the product is exact in float)
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "polar_device.h"
#include "polar_enc_device.h"
#include "polar_llr_device.h"

namespace bchk {

__global__ void __launch_bounds__(64) polar_genie_kernel(PolarGenieParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t gsm[];
    using pllr::wsync;
    const int lane = (int)threadIdx.x;
    const PolarEncTables &t = p.t;
    const int U = t.U, nl = t.nl, K = t.K;
    const PolarGenieLayout lo = polar_genie_layout(U, K, p.ssize, p.csize, p.osize, nl, p.tstates);
    float *chan = reinterpret_cast<float *>(gsm);
    float *S = reinterpret_cast<float *>(gsm + lo.o_S);
    uint8_t *C = gsm + lo.o_C;
    uint8_t *O = gsm + lo.o_O;
    uint64_t *rows = reinterpret_cast<uint64_t *>(gsm + lo.o_rows);  // [layer][row] bitmasks
    uint64_t *ib = reinterpret_cast<uint64_t *>(gsm + lo.o_ib);
    uint64_t *ua = reinterpret_cast<uint64_t *>(gsm + lo.o_u);
    const uint32_t *u32 = reinterpret_cast<const uint32_t *>(ua);
    for (int i = lane; i < kPolarMaxKernel * nl; i += 64) rows[i] = t.krows[i];
    auto Sof = [&](int, int lam) -> float * { return lam == 0 ? chan : S + p.soff[lam]; };
    auto Cof = [&](int, int lam) -> uint8_t * { return C + p.coff[lam]; };
    auto Oof = [&](int, int j) -> uint8_t * { return O + p.ooff[j]; };
    auto Fof = [&](int, int j) -> float * { return S + p.foff[j]; };  // named layers' state
    auto pathof = [](int) -> int { return 0; };  // one path
    const pllr::Trellis tr{p.tent, p.tbase, p.tlog, reinterpret_cast<float *>(gsm + lo.o_tm), p.tstates};
    const int lastsz = t.ksize[nl - 1];
    const int lastc = p.coff[nl];
    wsync();
    for (uint32_t cw = blockIdx.x; cw < p.B; cw += gridDim.x) {
        // ---- u, as the encoder forms it
        penc::pack_info(p.info_tx + (size_t)cw * K, K, ib, lane);
        wsync();
        penc::build_u(t, ib, ua, lane);
        uint8_t *urow = p.u + (size_t)cw * U;
        for (int i = lane; i < U; i += 64) urow[i] = (uint8_t)penc::ubit(u32, i);
        const float *y = p.llr + (size_t)cw * t.N;  // LoadLLRs (MixedKernelEncoder.cpp:181-207)
        for (int i = lane; i < U; i += 64) chan[i] = plist::chan_llr(p.symmap, y, i);
        wsync();
        float *drow = p.dec_llr + (size_t)cw * U;
        float keep = 0.0f;  // LLR of phase (phi & ~63) + lane
        for (int phi = 0; phi < U; ++phi) {
            // ---- IterativelyCalcS (KernelListEngine.cpp:370-447)
            int m = nl - 1;
            uint32_t pq = (uint32_t)phi;
            while (m > 0 && pq % (uint32_t)t.ksize[m] == 0) {
                pq /= (uint32_t)t.ksize[m];
                --m;
            }
            for (int j = m; j < nl; ++j) {
                const int loc = (j == m) ? (int)(pq % (uint32_t)t.ksize[j]) : 0;
                const int d = p.outer[j + 1], l = t.ksize[j];
                if (p.arikan[j]) {
                    pllr::arikan_llrs(j, loc, d, d, lane, pathof, Sof, Cof);
                    wsync();
                    continue;
                }
                if (p.named[j]) {
                    pllr::named_llrs(p.named[j], j, loc, d, d, lane, pathof, Sof, Cof, Fof, Oof);
                    wsync();
                    continue;
                }
                const uint64_t *kr = rows + kPolarMaxKernel * j;
                pllr::matrix_offsets(kr, j, l, loc, d, d, lane, pathof, Cof, Oof);
                wsync();
                if (p.trellis[j]) {
                    pllr::trellis_llrs(tr, j, l, loc, d, d, lane, pathof, Sof, Oof);
                    continue;
                }
                pllr::enum_llrs(kr, j, l, loc, d, d, lane, pathof, Sof, Oof);
                wsync();
            }
            const float lv = Sof(0, nl)[0];
            const int slot = phi & 63;
            if (lane == slot) keep = lv;
            if (slot == 63 || phi == U - 1) {
                if (lane <= slot) drow[(phi & ~63) + lane] = keep;
            }
            // ---- the TRUE u_phi, never the decision, then IterativelyUpdateC
            if (lane == 0) C[lastc + (phi % lastsz)] = (uint8_t)penc::ubit(u32, phi);
            wsync();
            pllr::update_c(rows, t.ksize, nl, phi, 1, lane, pathof, Cof);
        }
        wsync();  // the next word overwrites the buffers
    }
}

__global__ void __launch_bounds__(64) polar_genie_sum_kernel(const float *dec_llr, const uint8_t *u, uint32_t B, int U,
                                                             uint32_t rows_per, unsigned long long *err,
                                                             unsigned long long *soft) {
    const int phi = (int)(blockIdx.x * 64u + threadIdx.x);
    if (phi >= U) return;
    const uint64_t b0 = (uint64_t)blockIdx.y * rows_per;
    const uint64_t b1 = b0 + rows_per < (uint64_t)B ? b0 + rows_per : (uint64_t)B;
    unsigned long long e = 0;
    long long q = 0;
    for (uint64_t b = b0; b < b1; ++b) {
        const float v = dec_llr[b * (uint64_t)U + (uint64_t)phi];
        const bool one = u[b * (uint64_t)U + (uint64_t)phi] != 0;
        e += ((v < 0.0f) != one) ? 1ull : 0ull;
        const float s = one ? -v : v;
        const float c = s < -32768.0f ? -32768.0f : (s > 32768.0f ? 32768.0f : s);
        q += __float2ll_rn(c * 65536.0f);
    }
    if (e) atomicAdd(err + phi, e);
    if (q) atomicAdd(soft + phi, (unsigned long long)q);
}

hipError_t launch_polar_genie(const PolarGenieParams &p, int grid, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL(polar_genie_kernel, dim3(grid), dim3(64), lds, s, p);
    return hipGetLastError();
}

hipError_t launch_polar_genie_sum(const float *dec_llr, const uint8_t *u, uint32_t B, int U, uint64_t *err,
                                  int64_t *soft, hipStream_t s) {
    // at most 65535 workgroups along the words
    const uint64_t least = ((uint64_t)B + 65534u) / 65535u;
    const uint32_t rows_per = least > kGenieSumRows ? (uint32_t)least : kGenieSumRows;
    const dim3 grid((unsigned)((U + 63) / 64), (unsigned)(((uint64_t)B + rows_per - 1) / rows_per));
    hipLaunchKernelGGL(polar_genie_sum_kernel, grid, dim3(64), 0, s, dec_llr, u, B, U, rows_per,
                       reinterpret_cast<unsigned long long *>(err), reinterpret_cast<unsigned long long *>(soft));
    return hipGetLastError();
}

const void *polar_genie_kernel_ptr() { return reinterpret_cast<const void *>(&polar_genie_kernel); }

}  // namespace bchk
