// The stages of mdc_iq_ddc (iq_ddc.hip) and mdc_iq_resample (iq_resample.hip) -- the "widening", "oscillator", "mixer" and
// "filter" of include/mdc.h.  Both kernels use the loads, the table and the LDS geometry below; the DDC calls mix_tile and
// fir_output, the resampler carries its own copies of those two for a measured reason (see its file head): what is said of the
// stages here holds for both.  mdc_iq_extract (iq_extract.hip) calls both as well, once per (job, tile): a job's slice is the base
// pointer and the bound it hands mix_tile.
//
//   loads     the quad loads of the three sample formats (load_quad) and the oscillator table.
//   mix       mix_tile: each thread takes four adjacent pairs at a time (one unaligned 8- or 16-byte vector load; the capture's
//             last, partial quads pair by pair with bounds), widens them to 16-bit full scale, reads the oscillator word of
//             phi_n = phase0 + n step (mod 2^32: the low word of the 64-bit n suffices) from the table's copy in LDS, and
//             writes m = x e^{j phi} / 2 as int16 into two PLANAR LDS images (re, im): adjacent samples share a dword.
//   filter    fir_output: one lane per output, acc += dot2(m[s + 2i], m[s + 2i + 1]; tap pair i) with the packed 16-bit dot
//             product (v_dot2c_i32_i16), in groups of GROUP tap dwords, the taps zero-padded to whole groups; where a tap dword
//             comes from is the caller's (a callable).  s odd (the ODD instantiations): the output's first sample is the HIGH
//             half of its dword; the lane then forms each operand from two neighbouring dwords with v_alignbit (shift 16;
//             lanes with an even s shift by 0), the taps stay as they are.
//   LDS       a lane starts at dword s / 2: for a decimation of 64 every lane of a wave would sit on ONE bank.  The images
//             therefore skip one dword after every 32 (lds_slot(i) = i + i / 32): a stride of 32 dwords becomes 33.
// All sums are the exact integers of the definition: |I c - Q s| + 32768 < 2^31, |acc| <= 32767 sum|h| <= 32767 * 65535,
// |acc| + 8192 < 2^31 (int32 wraps nowhere, and a dot2 without clamp is plain modular arithmetic in any case).
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

// the mix stage of one tile: local pairs 0 .. 4 quads - 1 (the capture's in0 on) into the two planar images
template <int FMT>
__device__ __forceinline__ void mix_tile(const unsigned char* __restrict__ iq, long in0, long pairs, unsigned phase0, unsigned step, int quads,
                                         const unsigned* nco, unsigned* re, unsigned* im, int tid) {
    for (int q = tid; q < quads; q += kIqMixThreads) {
        const long n = in0 + 4 * (long)q;
        int I[4], Q[4], mr[4], mi[4];
        load_quad<FMT>(iq, n, pairs, I, Q);
        const unsigned phi = phase0 + (unsigned)(unsigned long)n * step;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned cs = nco[(phi + (unsigned)e * step) >> 20];
            const int c = (int)(short)(cs & 0xFFFFu), s = (int)(short)(cs >> 16);
            mr[e] = (I[e] * c - Q[e] * s + 32768) >> 16;
            mi[e] = (I[e] * s + Q[e] * c + 32768) >> 16;
        }
        const int a = lds_slot(2 * q), b = lds_slot(2 * q + 1);
        re[a] = ((unsigned)mr[0] & 0xFFFFu) | ((unsigned)mr[1] << 16);
        re[b] = ((unsigned)mr[2] & 0xFFFFu) | ((unsigned)mr[3] << 16);
        im[a] = ((unsigned)mi[0] & 0xFFFFu) | ((unsigned)mi[1] << 16);
        im[b] = ((unsigned)mi[2] & 0xFFFFu) | ((unsigned)mi[3] << 16);
    }
}

// one output, packed (re | im << 16): the local samples from 2 base + (sh >> 4) on against ngroups * GROUP tap dwords, tap(k)
// the k-th of them (sh = 16 for an odd start, else 0; only the ODD instantiation may be handed 16)
template <bool ODD, int GROUP, class Tap>
__device__ __forceinline__ unsigned fir_output(const unsigned* re, const unsigned* im, int base, unsigned sh, int ngroups, Tap tap) {
    int ar = 0, ai = 0;
    unsigned cr = 0, ci = 0;
    if (ODD) { cr = re[lds_slot(base)]; ci = im[lds_slot(base)]; }
    for (int g = 0; g < ngroups; ++g) {
#pragma unroll
        for (int u = 0; u < GROUP; ++u) {
            const unsigned tp = tap(GROUP * g + u);
            unsigned wr, wi;
            if (ODD) {
                const int idx = lds_slot(base + GROUP * g + u + 1);
                const unsigned nr = re[idx], ni = im[idx];
                wr = __builtin_amdgcn_alignbit(nr, cr, sh);
                wi = __builtin_amdgcn_alignbit(ni, ci, sh);
                cr = nr;
                ci = ni;
            } else {
                const int idx = lds_slot(base + GROUP * g + u);
                wr = re[idx];
                wi = im[idx];
            }
            ar = dot2(wr, tp, ar);
            ai = dot2(wi, tp, ai);
        }
    }
    const int r = sat16((ar + 8192) >> 14), i = sat16((ai + 8192) >> 14);
    return ((unsigned)r & 0xFFFFu) | ((unsigned)i << 16);
}

}  // namespace

}  // namespace mdc
