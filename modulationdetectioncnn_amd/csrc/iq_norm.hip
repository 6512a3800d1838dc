// mdc_iq_u8_windows_norm -- the level-normalising front-end between an SDR capture and the forward kernels (include/mdc.h):
// per window of 128 unsigned 8-bit (I,Q) pairs, optional DC removal, scaling to a fixed complex rms, and the window's exact
// integer statistics (sums, sum of squares, energy) for a power estimate / squelch.
//
// One wave per window, lane l = 4 consecutive bytes = (I[2l], Q[2l], I[2l+1], Q[2l+1]).  Everything up to the energy is
// integer arithmetic on the raw bytes b (s = 2b - 255 is never formed per sample for the sums):
//     sum_I b, sum_Q b          one v_dot4_u32_u8 against the byte masks 0x00010001 / 0x01000100 (both <= 32,640: packed
//                               into the two halves of ONE register for the reduction)
//     sum b^2                   one v_dot4_u32_u8 of the word with itself
//     wave reduction            two integers, six xor steps each
//     sum_i = 2 sum_I b - 32,640;  sum_sq = 4 sum b^2 - 1,020 (sum_I b + sum_Q b) + 256 * 255^2;  E as the header defines it
// The centred sample times 128, 128 s - sum, is an integer below 2^17: exact in f32.  x = (128 s - sum) * (level / sqrt(E))
// is then one conversion of E, one square root, one division and one multiplication, each correctly rounded (hipcc's
// default for f32 sqrt and division) -- tests/test_iq_norm_gpu.py derives its 2^-21 relative bound from exactly these.
// A wave takes two ADJACENT windows per step and a work-group 2 * kNormWaves consecutive ones, so both loads are in flight
// together, the frames leave as one contiguous 8 KiB run per work-group step, and with a small hop the windows' common bytes
// come from the CU's L1 after their first read.  Statistics alone at a small hop take iq_stats_run_kernel (below) instead.
// Vector memory only.
#include "mdc_internal.h"

namespace mdc {

namespace {

constexpr int kNormWaves = 4;
constexpr unsigned kSumOfMidpoints = 255u * 128u;            // sum over a row of the "255" in s = 2 b - 255
constexpr unsigned kSqOfMidpoints = 255u * 255u * 256u;      // 16,646,400

__device__ __forceinline__ unsigned load4_unaligned(const unsigned char* p) {      // (2-byte aligned at odd hops; see load8_unaligned)
    unsigned r;
    __builtin_memcpy(&r, p, 4);
    return r;
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += (unsigned)__shfl_xor((int)v, m, 64);
    return v;
}

// the window's record from its three byte sums (sum_I b, sum_Q b, sum b^2)
__device__ __forceinline__ int4 window_stats(unsigned sbi, unsigned sbq, unsigned b2, bool remove_dc) {
    const int sum_i = (int)(2u * sbi) - (int)kSumOfMidpoints, sum_q = (int)(2u * sbq) - (int)kSumOfMidpoints;
    const unsigned sum_sq = 4u * b2 - 1020u * (sbi + sbq) + kSqOfMidpoints;
    // 128 sum_sq < 2^31 and the two squares are at most 32,640^2 each: no step leaves 32 bits
    const unsigned energy = 128u * sum_sq - (remove_dc ? (unsigned)(sum_i * sum_i) + (unsigned)(sum_q * sum_q) : 0u);
    return make_int4(sum_i, sum_q, (int)sum_sq, (int)energy);
}

// the whole window's work for one wave; w = this lane's four bytes
template <bool FRAMES, bool STATS>
__device__ __forceinline__ void norm_window(unsigned w, long f, int lane, bool remove_dc, float level, float* __restrict__ x,
                                            mdc_iq_window_stats* __restrict__ stats) {
    const unsigned bi = __builtin_amdgcn_udot4(w, 0x00010001u, 0u, false);
    const unsigned bq = __builtin_amdgcn_udot4(w, 0x01000100u, 0u, false);
    const unsigned iq = wave_sum(bi | (bq << 16));
    const unsigned b2 = wave_sum(__builtin_amdgcn_udot4(w, w, 0u, false));
    const int4 st = window_stats(iq & 0xFFFFu, iq >> 16, b2, remove_dc);
    if (STATS && lane == 0) *reinterpret_cast<int4*>(stats + f) = st;
    if (FRAMES) {
        const int sum_i = st.x, sum_q = st.y;
        const unsigned energy = (unsigned)st.w;
        const float g = energy ? level / sqrtf((float)energy) : 0.f;      // a constant window (E = 0, all a = 0): zeros, never 0 / 0
        const int ci = remove_dc ? sum_i : 0, cq = remove_dc ? sum_q : 0;
        const int s0 = 2 * (int)(w & 0xFFu) - 255, s1 = 2 * (int)((w >> 8) & 0xFFu) - 255;
        const int s2 = 2 * (int)((w >> 16) & 0xFFu) - 255, s3 = 2 * (int)(w >> 24) - 255;
        float* row_i = x + f * kFrameFloats + 2 * lane;
        *reinterpret_cast<float2*>(row_i) = make_float2((float)(128 * s0 - ci) * g, (float)(128 * s2 - ci) * g);
        *reinterpret_cast<float2*>(row_i + kSamples) = make_float2((float)(128 * s1 - cq) * g, (float)(128 * s3 - cq) * g);
    }
}

template <bool FRAMES, bool STATS>
__global__ __launch_bounds__(64 * kNormWaves) void iq_norm_kernel(const unsigned char* __restrict__ iq, long n, long hop2, float level, int remove_dc,
                                                                 float* __restrict__ x, mdc_iq_window_stats* __restrict__ stats) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // (scalar loop control)
    const long step = (long)gridDim.x * (2 * kNormWaves);
    // f0 is uniform over the wave: the reductions see all 64 lanes of one window; windows past n are never read or written
    for (long f0 = (long)blockIdx.x * (2 * kNormWaves) + 2 * wave; f0 < n; f0 += step) {
        const bool two = f0 + 1 < n;
        const unsigned w0 = load4_unaligned(iq + hop2 * f0 + 4 * lane);
        const unsigned w1 = two ? load4_unaligned(iq + hop2 * (f0 + 1) + 4 * lane) : 0u;
        norm_window<FRAMES, STATS>(w0, f0, lane, remove_dc != 0, level, x, stats);
        if (two) norm_window<FRAMES, STATS>(w1, f0 + 1, lane, remove_dc != 0, level, x, stats);
    }
}

// Statistics only, windows that overlap by three quarters or more (hop <= kRunMaxHop): a work-group reads a RUN of 1,024
// pairs ONCE (8 bytes per thread), forms the running sums of I bytes, Q bytes and squares over the run -- four pairs in
// registers, a shuffle scan over the wave, the four waves' totals through LDS -- and every window the run holds is then the
// difference of two entries: hop pairs of work per window instead of 128.  Integer sums: the same record, bit for bit, as
// the wave-per-window kernel.  A run's windows are (1,024 - 128) / hop + 1; pairs past the capture's end count as zero and
// are only ever part of entries no window reads.
constexpr int kRunThreads = 256;
constexpr int kRunPairs = 4 * kRunThreads;
constexpr int kRunMaxHop = 32;

__device__ __forceinline__ unsigned wave_scan(unsigned v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned u = (unsigned)__shfl_up((int)v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

__global__ __launch_bounds__(kRunThreads) void iq_stats_run_kernel(const unsigned char* __restrict__ iq, long n, int hop, int remove_dc,
                                                                  mdc_iq_window_stats* __restrict__ stats) {
    __shared__ unsigned pre_i[kRunPairs + 1], pre_q[kRunPairs + 1], pre_2[kRunPairs + 1];
    __shared__ unsigned wave_tot[3][kRunThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int per_run = (kRunPairs - 128) / hop + 1;
    const long total_pairs = (long)hop * (n - 1) + 128;      // what the capture holds: nothing beyond it is read
    for (long w0 = (long)blockIdx.x * per_run; w0 < n; w0 += (long)gridDim.x * per_run) {
        const long p0 = w0 * hop + 4 * t;
        uint2 v = make_uint2(0u, 0u);
        if (p0 + 4 <= total_pairs) {
            v = load8_unaligned(iq + 2 * p0);
        } else {
            unsigned short h[4] = {0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (p0 + k < total_pairs) __builtin_memcpy(&h[k], iq + 2 * (p0 + k), 2);
            v = make_uint2((unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16));
        }
        unsigned ci[4], cq[4], c2[4];      // inclusive sums over this thread's four pairs
        unsigned ai = 0, aq = 0, a2 = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned pair = ((k < 2 ? v.x : v.y) >> (16 * (k & 1))) & 0xFFFFu;
            const unsigned bi = pair & 0xFFu, bq = pair >> 8;
            ai += bi; aq += bq; a2 += bi * bi + bq * bq;
            ci[k] = ai; cq[k] = aq; c2[k] = a2;
        }
        const unsigned si = wave_scan(ai, lane), sq = wave_scan(aq, lane), s2 = wave_scan(a2, lane);
        if (lane == 63) { wave_tot[0][wave] = si; wave_tot[1][wave] = sq; wave_tot[2][wave] = s2; }
        __syncthreads();      // (also: every read of the previous run's entries is done)
        unsigned oi = si - ai, oq = sq - aq, o2 = s2 - a2;      // sums over all pairs before this thread's
        for (int w = 0; w < wave; ++w) { oi += wave_tot[0][w]; oq += wave_tot[1][w]; o2 += wave_tot[2][w]; }
        if (t == 0) { pre_i[0] = 0u; pre_q[0] = 0u; pre_2[0] = 0u; }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            pre_i[4 * t + k + 1] = oi + ci[k];
            pre_q[4 * t + k + 1] = oq + cq[k];
            pre_2[4 * t + k + 1] = o2 + c2[k];
        }
        __syncthreads();
        for (int j = t; j < per_run && w0 + j < n; j += kRunThreads) {
            const int s = hop * j;
            *reinterpret_cast<int4*>(stats + w0 + j) =
                window_stats(pre_i[s + 128] - pre_i[s], pre_q[s + 128] - pre_q[s], pre_2[s + 128] - pre_2[s], remove_dc != 0);
        }
        __syncthreads();      // the entries (and wave_tot) are rewritten by the next run
    }
}

}  // namespace

int iq_norm_launch(const uint8_t* iq, int64_t n, int64_t hop, float level, int flags, float* x, mdc_iq_window_stats* stats, hipStream_t s) {
    if (n == 0) return MDC_OK;
    long grid = (n + 2 * kNormWaves - 1) / (2 * kNormWaves);
    if (grid > 16384) grid = 16384;
    const dim3 g((unsigned)grid), b(64 * kNormWaves);
    const int dc = (flags & MDC_IQ_REMOVE_DC) != 0;
    if (!x && hop <= kRunMaxHop) {
        const long per_run = (kRunPairs - 128) / hop + 1;
        long runs = (n + per_run - 1) / per_run;
        if (runs > 16384) runs = 16384;
        hipLaunchKernelGGL(iq_stats_run_kernel, dim3((unsigned)runs), dim3(kRunThreads), 0, s, iq, (long)n, (int)hop, dc, stats);
        MDC_HIP(hipGetLastError());
        return MDC_OK;
    }
    if (x && stats) hipLaunchKernelGGL((iq_norm_kernel<true, true>), g, b, 0, s, iq, (long)n, (long)(2 * hop), level, dc, x, stats);
    else if (x)     hipLaunchKernelGGL((iq_norm_kernel<true, false>), g, b, 0, s, iq, (long)n, (long)(2 * hop), level, dc, x, stats);
    else            hipLaunchKernelGGL((iq_norm_kernel<false, true>), g, b, 0, s, iq, (long)n, (long)(2 * hop), level, dc, x, stats);
    MDC_HIP(hipGetLastError());
    return MDC_OK;
}

}  // namespace mdc
