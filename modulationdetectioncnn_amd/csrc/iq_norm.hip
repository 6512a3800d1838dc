// mdc_iq_u8_windows_norm -- the level-normalising front-end between an SDR capture and the forward kernels (include/mdc.h):
// per window of 128 unsigned 8-bit (I,Q) pairs, optional DC removal, scaling to a fixed complex rms, and the window's exact
// integer statistics (sums, sum of squares, energy) for a power estimate / squelch.
//
// Frames, and statistics at hops above kRunMaxHop, come from the wave-per-window normaliser that all sample formats share
// (iq_formats.hip: its MDC_IQ_CU8 instantiation with the 32-bit record).  Statistics alone at a small hop take
// iq_stats_run_kernel (below) instead: another algorithm that leaves the same integers.  window_stats defines them from the
// three sums of a window's raw bytes b:
//     sum_i = 2 sum_I b - 32,640;  sum_sq = 4 sum b^2 - 1,020 (sum_I b + sum_Q b) + 256 * 255^2;  E as the header defines it.
// Vector memory only.
#include "mdc_internal.h"

namespace mdc {

namespace {

constexpr unsigned kSumOfMidpoints = 255u * 128u;            // sum over a row of the "255" in s = 2 b - 255
constexpr unsigned kSqOfMidpoints = 255u * 255u * 256u;      // 16,646,400

// the window's record from its three byte sums (sum_I b, sum_Q b, sum b^2)
__device__ __forceinline__ int4 window_stats(unsigned sbi, unsigned sbq, unsigned b2, bool remove_dc) {
    const int sum_i = (int)(2u * sbi) - (int)kSumOfMidpoints, sum_q = (int)(2u * sbq) - (int)kSumOfMidpoints;
    const unsigned sum_sq = 4u * b2 - 1020u * (sbi + sbq) + kSqOfMidpoints;
    // 128 sum_sq < 2^31 and the two squares are at most 32,640^2 each: no step leaves 32 bits
    const unsigned energy = 128u * sum_sq - (remove_dc ? (unsigned)(sum_i * sum_i) + (unsigned)(sum_q * sum_q) : 0u);
    return make_int4(sum_i, sum_q, (int)sum_sq, (int)energy);
}

// Statistics only, windows that overlap by three quarters or more (hop <= kRunMaxHop): a work-group reads a RUN of 1,024
// pairs ONCE (8 bytes per thread), forms the running sums of I bytes, Q bytes and squares over the run -- four pairs in
// registers, a shuffle scan over the wave, the four waves' totals through LDS -- and every window the run holds is then the
// difference of two entries: hop pairs of work per window instead of 128.  Integer sums: the same record, bit for bit, as
// the wave-per-window kernel's.  A run's windows are (1,024 - 128) / hop + 1; pairs past the capture's end count as zero and
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
    if (x || hop > kRunMaxHop) return iq_norm_wave_launch(iq, n, hop, level, flags, x, stats, s);
    const long per_run = (kRunPairs - 128) / hop + 1;
    long runs = (n + per_run - 1) / per_run;
    if (runs > kIqGridCap) runs = kIqGridCap;
    hipLaunchKernelGGL(iq_stats_run_kernel, dim3((unsigned)runs), dim3(kRunThreads), 0, s, iq, (long)n, (int)hop, (flags & MDC_IQ_REMOVE_DC) != 0, stats);
    MDC_HIP(hipGetLastError());
    return MDC_OK;
}

}  // namespace mdc
