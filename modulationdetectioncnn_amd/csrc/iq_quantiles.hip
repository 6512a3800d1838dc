// mdc_iq_spectrum_quantiles -- exact per-column order statistics of a (rows x nfft) float32 spectrogram on the device
// (include/mdc.h, "spectrum quantiles"; the numpy restatement is tests/iq_quantile_ref.py).  The call may allocate nothing, so a
// column's selection happens inside one work-group: an 8-bit radix select from the top byte down, on the values' bit patterns
// as unsigned integers.
//
//   tile      one work-group of 1024 threads owns kQuantTile adjacent columns and walks all rows of them: lane = column, so that a
//             row's segment is one contiguous read (kQuantTile * 4 bytes) and a wave covers 64 / kQuantTile rows; eight rows
//             are in flight per thread.  nfft / kQuantTile work-groups, at most one per CU at nfft = 4096: sixteen waves are what
//             keeps a CU's loads and LDS atomics busy (measured against 256 and 512 threads).
//   pass      per pass every value whose higher bytes equal a rank's prefix adds 1 to that rank's histogram of the pass's byte:
//             256 x kQuantTile 32-bit counters in LDS, [digit][column] (a wave's lanes are different columns: different banks;
//             the rows of one wave that share a column and a digit meet on one address), LDS atomic adds.  Then one thread per
//             (rank, column) walks the 256 counters, finds the digit that holds the rank, appends it to the prefix and
//             subtracts what lies below it from the rank.  After the pass of byte 0 the prefix is the answer.
//   ranks     the pass of the top byte is shared by all ranks (no prefix yet); the three passes below it take the ranks in
//             groups of kQuantGroup histograms, so that (0.5, hold) costs four walks over the tile, not seven.
//   order     counts are integers and the scan is a fixed walk: the same bits on every run; nothing of a column leaves its lane
//             but through its own counters.  A NaN or a negative pattern is ordered like any other unsigned integer.
// The matrix is read 1 + 3 ceil(nranks / kQuantGroup) times, the first time from HBM; a tile of 16 columns x 16,384 rows is
// 1 MiB and comes from L2 after that.  Vector memory for every store; the call only enqueues.  DESIGN.md 5.20.
#include "mdc_internal.h"

namespace mdc {

namespace {

constexpr int kQuantMinLog2 = 6, kQuantMaxLog2 = 12, kQuantMaxRanks = 8;
#ifndef MDC_QUANTILE_THREADS
#define MDC_QUANTILE_THREADS 1024      // the three macros exist for the A/B builds of tools/quantile_probe.py --lib
#endif
constexpr int kQuantThreads = MDC_QUANTILE_THREADS;
#ifndef MDC_QUANTILE_TILE
#define MDC_QUANTILE_TILE 16
#endif
constexpr int kQuantTile = MDC_QUANTILE_TILE;
constexpr int kQuantHistBytes = 48 * 1024;      // of the 64 KiB a work-group may declare; the rank state takes 64 * kQuantTile more
constexpr int kQuantGroupFit = kQuantHistBytes / (256 * kQuantTile * 4);
constexpr int kQuantGroup = kQuantGroupFit < 1 ? 1 : kQuantGroupFit > 4 ? 4 : kQuantGroupFit;
#ifndef MDC_QUANTILE_UNROLL
#define MDC_QUANTILE_UNROLL 8
#endif
constexpr int kQuantUnroll = MDC_QUANTILE_UNROLL;      // rows in flight per thread
static_assert(kQuantTile == 8 || kQuantTile == 16 || kQuantTile == 32, "a tile is 8, 16 or 32 columns");
static_assert(kQuantMaxRanks * kQuantTile <= kQuantThreads, "one thread per (rank, column) in the scan");

struct QuantRanks {      // travels with the launch, like mdc_iq_ddc's taps
    int n;
    unsigned rank[kQuantMaxRanks];
};

// fn(pattern) for every row of one column, this thread's rows r0, r0 + step, ...: kQuantUnroll loads in flight
template <class Fn>
__device__ __forceinline__ void quant_walk(const unsigned* __restrict__ col, long rows, long nfft, int r0, int step, Fn&& fn) {
    long r = r0;
    for (; r + (long)(kQuantUnroll - 1) * step < rows; r += (long)kQuantUnroll * step) {
        unsigned v[kQuantUnroll];
#pragma unroll
        for (int u = 0; u < kQuantUnroll; ++u) v[u] = col[(r + (long)u * step) * nfft];
#pragma unroll
        for (int u = 0; u < kQuantUnroll; ++u) fn(v[u]);
    }
    for (; r < rows; r += step) fn(col[r * nfft]);
}

// the digit of hist[.][c] that holds rank k (0-based among the counted values), and k less the counts below that digit.  The
// walk is unconditional -- 256 loads that depend on nothing, then compares -- and the counts sum to more than k, so a digit is found.
__device__ __forceinline__ void quant_scan(const unsigned (*hist)[kQuantTile], int c, unsigned k, unsigned& digit, unsigned& below) {
    unsigned cum = 0, d_sel = 255, b_sel = 0;
#pragma unroll 16
    for (int d = 0; d < 256; ++d) {
        const unsigned cnt = hist[d][c];
        if (k >= cum && k - cum < cnt) { d_sel = (unsigned)d; b_sel = cum; }
        cum += cnt;
    }
    digit = d_sel;
    below = b_sel;
}

__global__ __launch_bounds__(kQuantThreads) void iq_quantiles_kernel(const unsigned* __restrict__ power, long rows, int nfft, QuantRanks ranks,
                                                                    unsigned* __restrict__ out) {
    constexpr int W = kQuantTile, G = kQuantGroup, R = kQuantThreads / W;
    __shared__ unsigned hist[G][256][W];
    __shared__ unsigned prefix[kQuantMaxRanks][W];      // the bytes found so far, in place; the bytes below them 0
    __shared__ unsigned left[kQuantMaxRanks][W];        // the rank among the values that share the prefix
    const int tid = threadIdx.x, c = tid % W, r0 = tid / W;
    const long column = (long)blockIdx.x * W + c;
    const unsigned* col = power + column;
    const int n = ranks.n;

    // the top byte: one histogram for all ranks
    for (int i = tid; i < 256 * W; i += kQuantThreads) (&hist[0][0][0])[i] = 0u;
    __syncthreads();
    quant_walk(col, rows, nfft, r0, R, [&](unsigned v) { atomicAdd(&hist[0][v >> 24][c], 1u); });
    __syncthreads();
    if (tid < n * W) {
        const int i = tid / W;
        unsigned digit, below;
        quant_scan(hist[0], c, ranks.rank[i], digit, below);
        prefix[i][c] = digit << 24;
        left[i][c] = ranks.rank[i] - below;
    }
    __syncthreads();

    for (int shift = 16; shift >= 0; shift -= 8) {
        for (int g0 = 0; g0 < n; g0 += G) {
            const int ng = n - g0 < G ? n - g0 : G;
            for (int i = tid; i < ng * 256 * W; i += kQuantThreads) (&hist[0][0][0])[i] = 0u;
            unsigned pre[G];
#pragma unroll
            for (int j = 0; j < G; ++j) pre[j] = j < ng ? prefix[g0 + j][c] : 0u;
            __syncthreads();
            quant_walk(col, rows, nfft, r0, R, [&](unsigned v) {
                const unsigned digit = (v >> shift) & 255u;
#pragma unroll
                for (int j = 0; j < G; ++j)
                    if (j < ng && ((v ^ pre[j]) >> (shift + 8)) == 0u) atomicAdd(&hist[j][digit][c], 1u);
            });
            __syncthreads();
            if (tid < ng * W) {
                const int j = tid / W;
                unsigned digit, below;
                quant_scan(hist[j], c, left[g0 + j][c], digit, below);
                prefix[g0 + j][c] |= digit << shift;
                left[g0 + j][c] -= below;
            }
            __syncthreads();
        }
    }
    if (tid < n * W) out[(long)(tid / W) * nfft + column] = prefix[tid / W][c];
}

}  // namespace

}  // namespace mdc

using namespace mdc;

int mdc_iq_spectrum_quantiles(const float* power_dev, int64_t rows, int nfft, const int64_t* ranks_host, int nranks, float* out_dev, void* hip_stream) {
    const char* who = "mdc_iq_spectrum_quantiles";
    if (nranks < 0 || nranks > kQuantMaxRanks) { set_error("%s: nranks must be in 0..%d (got %d)", who, kQuantMaxRanks, nranks); return MDC_EINVAL; }
    if (pow2_log2(nfft, kQuantMinLog2, kQuantMaxLog2) < 0) { set_error("%s: nfft must be a power of two in %d..%d (got %d)", who, 1 << kQuantMinLog2, 1 << kQuantMaxLog2, nfft); return MDC_EINVAL; }
    if (rows < 1 || rows > 2147483647LL) { set_error("%s: rows must be in 1..2^31-1 (got %lld)", who, (long long)rows); return MDC_EINVAL; }
    int rc = iq_aligned(who, "power_dev", power_dev, 4);
    if (rc != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "out_dev", out_dev, 4)) != MDC_OK) return rc;
    if (nranks == 0) return MDC_OK;
    if (!power_dev || !out_dev || !ranks_host) { set_error("%s: null buffer", who); return MDC_EINVAL; }
    QuantRanks ranks{};
    ranks.n = nranks;
    for (int i = 0; i < nranks; ++i) {
        if (ranks_host[i] < 0 || ranks_host[i] >= rows) {
            set_error("%s: rank %d is %lld, outside 0..rows-1 = %lld", who, i, (long long)ranks_host[i], (long long)(rows - 1));
            return MDC_EINVAL;
        }
        ranks.rank[i] = (unsigned)ranks_host[i];
    }
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return guarded(who, [&]() -> int {
        hipLaunchKernelGGL(iq_quantiles_kernel, dim3((unsigned)(nfft / kQuantTile)), dim3(kQuantThreads), 0, s, reinterpret_cast<const unsigned*>(power_dev),
                           (long)rows, nfft, ranks, reinterpret_cast<unsigned*>(out_dev));
        MDC_HIP(hipGetLastError());
        return MDC_OK;
    });
}
