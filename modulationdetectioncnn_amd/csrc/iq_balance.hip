// mdc_iq_balance_stats / mdc_iq_balance -- measure and correct a receiver's I/Q imbalance and DC offset on the device, in exact
// integer arithmetic (include/mdc.h, "I/Q balance"; the numpy int64 restatement is tests/iq_balance_ref.py).  Two pointwise
// streams over the capture, through iq_mix.h's quad loader and its widening (but for the 8-bit statistics' whole groups):
//
//   stats     iq_balance_stats_kernel: the capture in blocks of B pairs, one work-group of 256 lanes per block and stride step
//             (grid cap kBalStatsGridCap).  The block's pairs up to the first 16-byte boundary go one per lane through the
//             loader's bounded path (the head); from there every lane takes 16 bytes a step, while whole 16-byte groups last;
//             the pairs left (fewer than a group) go one per lane again (the tail).  MDC_IQ_CI16's group is one quad of the
//             loader.  The 8-bit formats' group is eight pairs, and through the loader -- unpack, widen, five multiply-adds per
//             pair -- the kernel ran at 0.46 .. 0.50 of a copy's byte rate, bound by the vector ALU; their groups are therefore
//             one aligned 16-byte load of RAW bytes and five packed byte dot products (v_dot4_u32_u8) per dword: with b the
//             byte (MDC_IQ_CI8: the sample + 128, one XOR per dword) and u = alpha b - beta the sample in units of 2^s
//             (MDC_IQ_CU8: alpha 2, beta 255, s 7; MDC_IQ_CI8: alpha 1, beta 128, s 8), sum u = alpha sum b - beta n,
//             sum u^2 = alpha^2 sum b^2 - 2 alpha beta sum b + beta^2 n, sum u v = alpha^2 sum b_i b_q - alpha beta (sum b_i +
//             sum b_q) + beta^2 n, folded once per lane and block.  A lane's share is at most 4096 + 1 + 1 pairs (B <= 2^20
//             over 256 lanes in whole groups, one head and one tail pair), hence per lane:
//               sum x, sum y         |.| <= 4098 * 2^15 < 2^28: int32, every format
//               8-bit formats        sum b^2, sum b_i b_q <= 4098 * 255^2 < 2^28, and every term of the fold -- at most
//                                    4 * 4098 * 255^2 -- < 2^31: int32 throughout, shifted by s or 2 s once at the end
//               MDC_IQ_CI16          x^2, |x y| <= 2^30, 4098 of them < 2^43: int64; two squares fit one unsigned dword
//                                    (<= 2^31) and enter the 64-bit sum together
//             Then the five sums as int64 across the wave by shuffles, across the four waves through LDS, and lane 0 writes the
//             block's row.  Every sum is exact, so the order is free and runs are bit-identical.
//   balance   iq_balance_kernel: four pairs per lane, grid-stride (grid cap kBalGridCap); the six coefficients are kernel
//             ARGUMENTS.  |a| <= 65536 and |m_i0| + |m_i1| <= 32767 keep m a + m' b + 8192 inside int32 (mdc.h); each factor
//             fits 24 bits, so the products are v_mul_i32_i24.  Whole quads leave as four dwords, the last pairs one by one.
// Both calls only enqueue; vector memory for every store.
#include "iq_mix.h"

namespace mdc {

namespace {

constexpr int kBalThreads = kIqMixThreads;
constexpr long kBalStatsGridCap = 2048;      // work-groups (blocks in flight); beyond it the kernel strides (_cabi.BALANCE_STATS_GRID_CAP)
constexpr long kBalGridCap = 2048;           // work-groups of 1024 pairs (_cabi.BALANCE_GRID_CAP)
constexpr int64_t kBalMinBlock = 64, kBalMaxBlock = (int64_t)1 << 20;

template <int FMT> struct BalSums {
    static constexpr bool kWide = FMT == MDC_IQ_CI16;
    static constexpr int kShift = FMT == MDC_IQ_CU8 ? 7 : FMT == MDC_IQ_CI8 ? 8 : 0;      // x = u << kShift, exactly
    static constexpr int kAlpha = FMT == MDC_IQ_CU8 ? 2 : 1, kBeta = FMT == MDC_IQ_CU8 ? 255 : 128;      // u = kAlpha b - kBeta
    using Acc = typename std::conditional<kWide, long, int>::type;
    int sx = 0, sy = 0;
    Acc sxx = 0, syy = 0, sxy = 0;
    unsigned bi = 0, bq = 0, bii = 0, bqq = 0, biq = 0;      // 8-bit formats: the raw groups' byte sums, and their pairs
    int braw = 0;

    __device__ __forceinline__ void add(const int (&I)[4], const int (&Q)[4]) {
        if constexpr (kWide) {
#pragma unroll
            for (int e = 0; e < 4; e += 2) {
                sx += I[e] + I[e + 1];
                sy += Q[e] + Q[e + 1];
                sxx += (long)((unsigned)__mul24(I[e], I[e]) + (unsigned)__mul24(I[e + 1], I[e + 1]));
                syy += (long)((unsigned)__mul24(Q[e], Q[e]) + (unsigned)__mul24(Q[e + 1], Q[e + 1]));
                sxy += (long)__mul24(I[e], Q[e]);
                sxy += (long)__mul24(I[e + 1], Q[e + 1]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int u = I[e] >> kShift, v = Q[e] >> kShift;
                sx += u;
                sy += v;
                sxx += __mul24(u, u);
                syy += __mul24(v, v);
                sxy += __mul24(u, v);
            }
        }
    }

    // eight pairs as they lie in memory (8-bit formats): byte 0 and 2 of a dword are I, byte 1 and 3 are Q
    __device__ __forceinline__ void add_raw(const uint4& g) {
        const unsigned v[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned w = FMT == MDC_IQ_CI8 ? v[k] ^ 0x80808080u : v[k];
            const unsigned wi = w & 0x00FF00FFu, wq = w & 0xFF00FF00u;
            bi = __builtin_amdgcn_udot4(w, 0x00010001u, bi, false);
            bq = __builtin_amdgcn_udot4(w, 0x01000100u, bq, false);
            bii = __builtin_amdgcn_udot4(wi, w, bii, false);
            bqq = __builtin_amdgcn_udot4(wq, w, bqq, false);
            biq = __builtin_amdgcn_udot4(wi, w >> 8, biq, false);      // I0 Q0 + I1 Q1: w >> 8 has Q under I
        }
        braw += 8;
    }

    // the raw groups' sums into the sums over u (file head: every term stays inside int32)
    __device__ __forceinline__ void fold() {
        if constexpr (!kWide) {
            const int si = (int)bi, sq = (int)bq, n = braw;
            sx += kAlpha * si - kBeta * n;
            sy += kAlpha * sq - kBeta * n;
            sxx += kAlpha * kAlpha * (int)bii - 2 * kAlpha * kBeta * si + kBeta * kBeta * n;
            syy += kAlpha * kAlpha * (int)bqq - 2 * kAlpha * kBeta * sq + kBeta * kBeta * n;
            sxy += kAlpha * kAlpha * (int)biq - kAlpha * kBeta * (si + sq) + kBeta * kBeta * n;
        }
    }
};

__device__ __forceinline__ long wave_sum64(long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

template <int FMT>
__global__ __launch_bounds__(kBalThreads) void iq_balance_stats_kernel(const unsigned char* __restrict__ iq, long pairs, long B, long nblocks,
                                                                       long* __restrict__ sums) {
    constexpr int kPB = Quad<FMT>::kPairBytes;
    constexpr int kStep = 16 / kPB;      // pairs in a lane's 16 bytes
    __shared__ long part[kBalThreads / 64][5];
    const int tid = threadIdx.x;
    for (long b = blockIdx.x; b < nblocks; b += gridDim.x) {
        const long p0 = b * B, p1 = p0 + B < pairs ? p0 + B : pairs;
        // pairs before the first 16-byte boundary at or after the block's first byte (iq itself is aligned to a pair only)
        const unsigned long addr = reinterpret_cast<unsigned long>(iq) + (unsigned long)p0 * kPB;
        long head = (long)((0 - addr) & 15ul) / kPB;
        if (head > p1 - p0) head = p1 - p0;
        const long a0 = p0 + head, a1 = a0 + (p1 - a0) / kStep * kStep;      // whole 16-byte groups: [a0, a1)
        BalSums<FMT> s;
        int I[4], Q[4];
        if (tid < head) {      // the bounded path with one pair inside the bound: pair p0 + tid alone, three zeros
            load_quad<FMT>(iq, p0 + tid, p0 + tid + 1, I, Q);
            s.add(I, Q);
        }
        if (tid < p1 - a1) {      // the tail, fewer than kStep pairs, likewise
            load_quad<FMT>(iq, a1 + tid, a1 + tid + 1, I, Q);
            s.add(I, Q);
        }
#pragma unroll 4
        for (long n = a0 + (long)tid * kStep; n < a1; n += (long)kBalThreads * kStep) {
            if constexpr (FMT == MDC_IQ_CI16) {
                load_quad<FMT>(iq, n, n + 4, I, Q);      // a whole quad by construction: the loader's bound check folds away, and
                s.add(I, Q);                             // with it the branch that kept the unrolled steps' loads from overlapping
            } else {
                s.add_raw(*reinterpret_cast<const uint4*>(iq + n * kPB));      // 16-byte aligned: a0 is, and n - a0 is whole groups
            }
        }
        s.fold();
        constexpr int sh = BalSums<FMT>::kShift;
        long r[5] = {(long)s.sx << sh, (long)s.sy << sh, (long)s.sxx << 2 * sh, (long)s.syy << 2 * sh, (long)s.sxy << 2 * sh};
#pragma unroll
        for (int k = 0; k < 5; ++k) r[k] = wave_sum64(r[k]);
        __syncthreads();      // the previous block's row has been read
        if ((tid & 63) == 0) {
#pragma unroll
            for (int k = 0; k < 5; ++k) part[tid >> 6][k] = r[k];
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < 5; ++k) sums[b * 5 + k] = part[0][k] + part[1][k] + part[2][k] + part[3][k];
        }
    }
}

template <int FMT>
__global__ __launch_bounds__(kBalThreads) void iq_balance_kernel(const unsigned char* __restrict__ iq, long pairs, const mdc_iq_balance_coeffs c,
                                                                 unsigned* __restrict__ out) {
    const long stride = (long)gridDim.x * kBalThreads * 4;
    for (long n = ((long)blockIdx.x * kBalThreads + threadIdx.x) * 4; n < pairs; n += stride) {
        int I[4], Q[4];
        load_quad<FMT>(iq, n, pairs, I, Q);
        unsigned w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int a = I[e] - c.dc_i, b = Q[e] - c.dc_q;
            const int oi = sat16((__mul24(c.m00, a) + __mul24(c.m01, b) + 8192) >> 14);
            const int oq = sat16((__mul24(c.m10, a) + __mul24(c.m11, b) + 8192) >> 14);
            w[e] = ((unsigned)oi & 0xFFFFu) | ((unsigned)oq << 16);
        }
        if (n + 4 <= pairs) {
            const uint4 v = make_uint4(w[0], w[1], w[2], w[3]);
            __builtin_memcpy(out + n, &v, sizeof(v));
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (n + e < pairs) out[n + e] = w[e];
        }
    }
}

int balance_block_check(const char* who, int64_t pairs, int64_t B) {
    if (pairs < 0) { set_error("%s: negative pair count", who); return MDC_EINVAL; }
    if (B < kBalMinBlock || B > kBalMaxBlock) {
        set_error("%s: block_pairs must be in %lld..%lld (got %lld)", who, (long long)kBalMinBlock, (long long)kBalMaxBlock, (long long)B);
        return MDC_EINVAL;
    }
    return MDC_OK;
}

int64_t balance_blocks(int64_t pairs, int64_t B) { return pairs / B + (pairs % B != 0); }

template <int FMT>
int balance_stats_launch(const unsigned char* iq, int64_t pairs, int64_t B, int64_t nblocks, int64_t* sums, hipStream_t s) {
    const dim3 g((unsigned)(nblocks < kBalStatsGridCap ? nblocks : kBalStatsGridCap)), b(kBalThreads);
    hipLaunchKernelGGL((iq_balance_stats_kernel<FMT>), g, b, 0, s, iq, (long)pairs, (long)B, (long)nblocks, reinterpret_cast<long*>(sums));
    MDC_HIP(hipGetLastError());
    return MDC_OK;
}

template <int FMT>
int balance_launch(const unsigned char* iq, int64_t pairs, const mdc_iq_balance_coeffs& c, int16_t* out, hipStream_t s) {
    const long groups = (pairs + 4 * kBalThreads - 1) / (4 * kBalThreads);
    const dim3 g((unsigned)(groups < kBalGridCap ? groups : kBalGridCap)), b(kBalThreads);
    hipLaunchKernelGGL((iq_balance_kernel<FMT>), g, b, 0, s, iq, (long)pairs, c, reinterpret_cast<unsigned*>(out));
    MDC_HIP(hipGetLastError());
    return MDC_OK;
}

}  // namespace

}  // namespace mdc

using namespace mdc;

int64_t mdc_iq_balance_blocks(int64_t pairs_in, int64_t block_pairs) {
    const int rc = balance_block_check("mdc_iq_balance_blocks", pairs_in, block_pairs);
    return rc != MDC_OK ? (int64_t)rc : balance_blocks(pairs_in, block_pairs);
}

int mdc_iq_balance_stats(const void* iq_dev, int format, int64_t pairs_in, int64_t block_pairs, int64_t* sums_dev, int64_t nblocks,
                         void* hip_stream) {
    int rc = iq_format_check("mdc_iq_balance_stats", format, 1);
    if (rc != MDC_OK) return rc;
    if ((rc = balance_block_check("mdc_iq_balance_stats", pairs_in, block_pairs)) != MDC_OK) return rc;
    if (nblocks != balance_blocks(pairs_in, block_pairs)) {
        set_error("mdc_iq_balance_stats: nblocks is %lld, mdc_iq_balance_blocks gives %lld", (long long)nblocks,
                  (long long)balance_blocks(pairs_in, block_pairs));
        return MDC_EINVAL;
    }
    if ((rc = iq_pair_aligned("mdc_iq_balance_stats", "iq_dev", format, iq_dev)) != MDC_OK) return rc;
    if ((rc = iq_aligned("mdc_iq_balance_stats", "sums_dev", sums_dev, 8)) != MDC_OK) return rc;
    if (pairs_in == 0) return MDC_OK;
    if (!iq_dev || !sums_dev) { set_error("mdc_iq_balance_stats: null buffer"); return MDC_EINVAL; }
    const unsigned char* p = static_cast<const unsigned char*>(iq_dev);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return guarded("mdc_iq_balance_stats", [&]() -> int {
        return with_format(format, [&](auto fmt) { return balance_stats_launch<decltype(fmt)::value>(p, pairs_in, block_pairs, nblocks, sums_dev, s); });
    });
}

int mdc_iq_balance(const void* iq_dev, int format, int64_t pairs_in, const mdc_iq_balance_coeffs* coeffs_host, int16_t* out_dev,
                   void* hip_stream) {
    int rc = iq_format_check("mdc_iq_balance", format, 1);
    if (rc != MDC_OK) return rc;
    if (pairs_in < 0) { set_error("mdc_iq_balance: negative pair count"); return MDC_EINVAL; }
    if (!coeffs_host) { set_error("mdc_iq_balance: null coefficients"); return MDC_EINVAL; }
    const mdc_iq_balance_coeffs c = *coeffs_host;
    if (c.dc_i < -32768 || c.dc_i > 32768 || c.dc_q < -32768 || c.dc_q > 32768) {
        set_error("mdc_iq_balance: dc_i and dc_q must lie in -32768..32768 (got %d, %d)", c.dc_i, c.dc_q);
        return MDC_EINVAL;
    }
    auto mag = [](int32_t v) { return v < 0 ? -(long)v : (long)v; };
    const long row0 = mag(c.m00) + mag(c.m01), row1 = mag(c.m10) + mag(c.m11);
    if (row0 > 32767 || row1 > 32767) {
        set_error("mdc_iq_balance: a row's absolute values sum to %ld; at most 32767 keeps the 32-bit accumulation exact", row0 > row1 ? row0 : row1);
        return MDC_EINVAL;
    }
    if ((rc = iq_pair_aligned("mdc_iq_balance", "iq_dev", format, iq_dev)) != MDC_OK) return rc;
    if ((rc = iq_aligned("mdc_iq_balance", "output", out_dev, 4)) != MDC_OK) return rc;
    if (pairs_in == 0) return MDC_OK;
    if (!iq_dev || !out_dev) { set_error("mdc_iq_balance: null buffer"); return MDC_EINVAL; }
    const uintptr_t in0 = reinterpret_cast<uintptr_t>(iq_dev), out0 = reinterpret_cast<uintptr_t>(out_dev);
    const uintptr_t in_bytes = (uintptr_t)pairs_in * (format == MDC_IQ_CI16 ? 4 : 2), out_bytes = (uintptr_t)pairs_in * 4;
    if (in0 < out0 + out_bytes && out0 < in0 + in_bytes) { set_error("mdc_iq_balance: output must not overlap the input"); return MDC_EINVAL; }
    const unsigned char* p = static_cast<const unsigned char*>(iq_dev);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return guarded("mdc_iq_balance", [&]() -> int {
        return with_format(format, [&](auto fmt) { return balance_launch<decltype(fmt)::value>(p, pairs_in, c, out_dev, s); });
    });
}
