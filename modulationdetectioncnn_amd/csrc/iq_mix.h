// What the mix stages of mdc_iq_ddc (iq_ddc.hip) and mdc_iq_resample (iq_resample.hip) share -- the "widening", "oscillator"
// and "mixer" of include/mdc.h: the quad loads of the three sample formats, the oscillator table, the packed 16-bit dot
// product, and the geometry of the two PLANAR int16 LDS images (re, im) in which adjacent samples share a dword.  The images
// skip one dword after every 32 (lds_slot): lanes whose outputs start 32 dwords apart would otherwise sit on ONE bank.
// Everything here has internal linkage: each translation unit that includes it carries its own copy of the table.
#pragma once
#include "mdc_internal.h"

namespace mdc {

namespace {

constexpr int kIqMixThreads = 256;
constexpr int kIqTilePairs = 8192;       // input pairs a tile spans at most
constexpr int kIqPadPairs = 32;          // beyond them: what zero-padded tap groups (and the odd-start look-ahead) still read
constexpr int kNcoEntries = 4096;

__host__ __device__ constexpr int lds_slot(int i) { return i + (i >> 5); }
constexpr int kPlaneDwords = lds_slot((kIqTilePairs + kIqPadPairs) / 2) + 1;

__device__ const unsigned d_nco[kNcoEntries] = {
#include "iq_ddc_nco_table.h"
};

typedef short short2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int dot2(unsigned a, unsigned b, int c) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, a), __builtin_bit_cast(short2v, b), c, false);
}

template <int FMT> struct Quad { using type = uint2; static constexpr int kPairBytes = 2; };
template <> struct Quad<MDC_IQ_CI16> { using type = uint4; static constexpr int kPairBytes = 4; };

template <int FMT> __device__ __forceinline__ int widen(int raw) {      // raw: the byte (CU8) or the signed sample
    return FMT == MDC_IQ_CU8 ? (2 * raw - 255) * 128 : FMT == MDC_IQ_CI8 ? raw * 256 : raw;
}

// the widened samples of pairs n .. n+3 (I[e], Q[e]); pairs at or beyond `pairs` read nothing and are zero
template <int FMT>
__device__ __forceinline__ void load_quad(const unsigned char* __restrict__ iq, long n, long pairs, int (&I)[4], int (&Q)[4]) {
    constexpr int kPB = Quad<FMT>::kPairBytes;
    if (n + 4 <= pairs) {
        typename Quad<FMT>::type w;
        __builtin_memcpy(&w, iq + n * kPB, sizeof(w));
        if constexpr (FMT == MDC_IQ_CI16) {
            const unsigned v[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) { I[e] = (int)(short)(v[e] & 0xFFFFu); Q[e] = (int)(short)(v[e] >> 16); }
        } else {
            const unsigned v[2] = {w.x, w.y};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned bi = (v[e >> 1] >> (16 * (e & 1))) & 0xFFu, bq = (v[e >> 1] >> (16 * (e & 1) + 8)) & 0xFFu;
                I[e] = widen<FMT>(FMT == MDC_IQ_CU8 ? (int)bi : (int)(signed char)bi);
                Q[e] = widen<FMT>(FMT == MDC_IQ_CU8 ? (int)bq : (int)(signed char)bq);
            }
        }
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        I[e] = Q[e] = 0;
        if (n + e < pairs) {
            const unsigned char* p = iq + (n + e) * kPB;
            if constexpr (FMT == MDC_IQ_CI16) {
                unsigned v;
                __builtin_memcpy(&v, p, 4);
                I[e] = (int)(short)(v & 0xFFFFu);
                Q[e] = (int)(short)(v >> 16);
            } else {
                I[e] = widen<FMT>(FMT == MDC_IQ_CU8 ? (int)p[0] : (int)(signed char)p[0]);
                Q[e] = widen<FMT>(FMT == MDC_IQ_CU8 ? (int)p[1] : (int)(signed char)p[1]);
            }
        }
    }
}

__device__ __forceinline__ int sat16(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

}  // namespace

}  // namespace mdc
