// mdc_iq_spectrogram_cfar -- a local noise floor for every cell of a (rows x nfft) float32 spectrogram: an order statistic of the
// cell's training set, the cells of a rectangle around it minus a guard rectangle (2-D order-statistic CFAR), and the ratio of
// the cell to that floor (include/mdc.h, "spectrogram CFAR"; the numpy restatement is tests/iq_cfar_ref.py).
//
// Everything works on CENTRED columns c = (k + nfft/2) mod nfft = k ^ (nfft/2).  One launch, one work-group per tile of
// kCfarTileRows x kCfarTileCols centred cells:
//   load     the tile plus a halo of train_rows rows above and below and train_bins columns left and right goes into LDS as 32-bit
//            patterns, de-rotated to centred order on the way in.  A halo position outside the spectrogram holds 0xFFFFFFFF.
//   select   a lane owns kCfarLaneCells cells of one column in consecutive rows (a wave: 64 adjacent columns of the same rows).  The
//            order statistic is built bit by bit from the top: with `cand` = the answer so far with the next bit set, the bit
//            stays iff #{t in T : t < cand} <= pos -- the largest x with #{t < x} <= pos is the pattern at position pos of the
//            ascending order, an element of T by construction.  The count is (window) - (guard), each a walk over a rectangle in
//            LDS; a word that is read is compared for all the lane's cells whose rectangle holds its row (a wave-uniform
//            choice, made by zeroing the cell's `cand` for that row: nothing is < 0).  0xFFFFFFFF is < no cand, so the halo
//            outside the spectrogram is never counted and border tiles run the same code as interior ones: the cut-off window
//            enters only through n and pos, which are integer functions of (r, c, rows, nfft).
//   store    floor and ratio = power / floor (one IEEE division) at the cell's natural position: the only global writes.
// Loop bounds are stated at the loops.  No atomics, no work-group waits for another, nothing is summed in floating point: the same
// bits on every run.  All stores are vector stores from plain C++.  LDS: (kCfarTileRows + 2 train_rows) x (kCfarTileCols +
// 2 train_bins) words, sized per launch -- 16 KB at the defaults (8, 32), 60 KB at the maxima (16, 128).
//
// Cost per lane (four cells) and bit: (2 train_rows + 4) x (2 train_bins + 1) + (2 guard_rows + 4) x (2 guard_bins + 1) LDS reads,
// each followed by a compare and an add per cell: 1,436 reads at the defaults.  Measured bound: VALU issue.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; no kernel spills, no scratch):
//   kernel            VGPR  SGPR  LDS bytes          threads
//   iq_cfar_kernel      57    63  per launch (above)     256
#include "mdc_internal.h"

namespace mdc {

namespace {

constexpr int kCfarMinLog2 = 6, kCfarMaxLog2 = 12, kCfarMaxTrainRows = 16, kCfarMaxTrainBins = 128;
constexpr int kCfarTileRows = 16, kCfarTileCols = 64, kCfarLaneCells = 4;      // kCfarTileCols divides every nfft
constexpr int kCfarThreads = kCfarTileCols * (kCfarTileRows / kCfarLaneCells);
constexpr unsigned kCfarOutside = 0xFFFFFFFFu, kCfarNaN = 0x7FC00000u;
static_assert(kCfarTileCols == 64, "a wave is 64 adjacent columns");
static_assert((kCfarTileRows + 2 * kCfarMaxTrainRows) * (kCfarTileCols + 2 * kCfarMaxTrainBins) * 4 <= 65536, "the tile and its halo fit 64 KB of LDS");

// #{t < cand[j]} over the rectangle of `nrows` x `ncols` words at p (row stride `stride`), for every cell j whose own rectangle --
// rows j .. j + span of it -- holds the row.  bound: nrows <= 2 * 16 + 4 rows of ncols <= 257 words.
__device__ __forceinline__ void cfar_count(const unsigned* p, int stride, int nrows, int ncols, int span, const unsigned (&cand)[kCfarLaneCells],
                                           unsigned (&cnt)[kCfarLaneCells]) {
    for (int u = 0; u < nrows; ++u, p += stride) {
        unsigned c[kCfarLaneCells];
#pragma unroll
        for (int j = 0; j < kCfarLaneCells; ++j) {
            c[j] = (u >= j && u <= j + span) ? cand[j] : 0u;      // wave-uniform
            asm volatile("" : "+v"(c[j]));      // (keeps the choice out of the inner loop: one compare and one add per word and cell there)
        }
#pragma unroll 8
        for (int x = 0; x < ncols; ++x) {
            const unsigned t = p[x];
#pragma unroll
            for (int j = 0; j < kCfarLaneCells; ++j) cnt[j] += t < c[j] ? 1u : 0u;
        }
    }
}

__global__ __launch_bounds__(kCfarThreads) void iq_cfar_kernel(const unsigned* __restrict__ power, int rows, int nfft, int tiles_c, int tr, int tb, int gr,
                                                              int gb, int rank, unsigned* __restrict__ floor_out, float* __restrict__ ratio_out) {
    extern __shared__ unsigned cfar_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = nfft >> 1;
    const int r0 = (int)(blockIdx.x / (unsigned)tiles_c) * kCfarTileRows, c0 = (int)(blockIdx.x % (unsigned)tiles_c) * kCfarTileCols;
    const int W = kCfarTileCols + 2 * tb, H = kCfarTileRows + 2 * tr;
    // LDS (lr, lc) is the cell (r0 - tr + lr, c0 - tb + lc).  bound: H * W <= 48 * 320 words, 60 per thread
    for (int l = tid; l < H * W; l += kCfarThreads) {
        const int lr = l / W, lc = l - lr * W, r = r0 - tr + lr, c = c0 - tb + lc;
        unsigned v = kCfarOutside;
        if (r >= 0 && r < rows && c >= 0 && c < nfft) v = power[(size_t)r * nfft + (c ^ half)];
        cfar_lds[l] = v;
    }
    __syncthreads();
    // my cells: rows rb + j, column c; in LDS rows wave * 4 + j + tr, column lane + tb
    const int rb = r0 + wave * kCfarLaneCells, c = c0 + lane;
    const int clo = max(c - tb, 0), chi = min(c + tb, nfft - 1), gclo = max(c - gb, 0), gchi = min(c + gb, nfft - 1);
    unsigned pos[kCfarLaneCells], ans[kCfarLaneCells];
    bool none[kCfarLaneCells];
#pragma unroll
    for (int j = 0; j < kCfarLaneCells; ++j) {
        const int r = min(rb + j, rows - 1);      // (a row past the end computes its neighbour's numbers and stores nothing)
        const int n = (min(r + tr, rows - 1) - max(r - tr, 0) + 1) * (chi - clo + 1) - (min(r + gr, rows - 1) - max(r - gr, 0) + 1) * (gchi - gclo + 1);
        none[j] = n <= 0;
        pos[j] = n > 0 ? (unsigned)(((long long)(n - 1) * rank) / 1000) : 0u;
        ans[j] = 0u;
    }
    const unsigned* win = cfar_lds + (wave * kCfarLaneCells) * W + lane;                        // rows [rb - tr ..], columns [c - tb ..]
    const unsigned* guard = cfar_lds + (wave * kCfarLaneCells + tr - gr) * W + lane + tb - gb;      // rows [rb - gr ..], columns [c - gb ..]
    for (int b = 31; b >= 0; --b) {      // bound: 32 bits
        unsigned cand[kCfarLaneCells], in[kCfarLaneCells], out[kCfarLaneCells];
#pragma unroll
        for (int j = 0; j < kCfarLaneCells; ++j) { cand[j] = ans[j] | (1u << b); in[j] = 0u; out[j] = 0u; }
        cfar_count(win, W, 2 * tr + kCfarLaneCells, 2 * tb + 1, 2 * tr, cand, in);
        cfar_count(guard, W, 2 * gr + kCfarLaneCells, 2 * gb + 1, 2 * gr, cand, out);
#pragma unroll
        for (int j = 0; j < kCfarLaneCells; ++j)
            if (in[j] - out[j] <= pos[j]) ans[j] = cand[j];
    }
#pragma unroll
    for (int j = 0; j < kCfarLaneCells; ++j) {
        const int r = rb + j;
        if (r >= rows) continue;
        const unsigned f = none[j] ? 0x7F800000u : ans[j];
        const size_t at = (size_t)r * nfft + (c ^ half);
        if (floor_out) floor_out[at] = f;
        if (ratio_out) {
            const float q = __uint_as_float(cfar_lds[(wave * kCfarLaneCells + j + tr) * W + lane + tb]) / __uint_as_float(f);
            ratio_out[at] = q != q ? __uint_as_float(kCfarNaN) : q;      // IEEE leaves a NaN's sign and payload open: the header names one
        }
    }
}

}  // namespace

}  // namespace mdc

using namespace mdc;

int mdc_iq_spectrogram_cfar(const float* power_dev, int64_t rows, int nfft, int train_rows, int train_bins, int guard_rows, int guard_bins,
                            int rank_permille, float* floor_dev, float* ratio_dev, void* hip_stream) {
    const char* who = "mdc_iq_spectrogram_cfar";
    if (pow2_log2(nfft, kCfarMinLog2, kCfarMaxLog2) < 0) { set_error("%s: nfft must be a power of two in %d..%d (got %d)", who, 1 << kCfarMinLog2, 1 << kCfarMaxLog2, nfft); return MDC_EINVAL; }
    if (rows < 1 || rows > 2147483647LL / nfft) { set_error("%s: rows must be >= 1 and rows * nfft <= 2^31-1 (got %lld)", who, (long long)rows); return MDC_EINVAL; }
    if (guard_rows < 0 || guard_rows > train_rows || train_rows > kCfarMaxTrainRows) { set_error("%s: 0 <= guard_rows <= train_rows <= %d (got %d, %d)", who, kCfarMaxTrainRows, guard_rows, train_rows); return MDC_EINVAL; }
    if (guard_bins < 0 || guard_bins > train_bins || train_bins > kCfarMaxTrainBins) { set_error("%s: 0 <= guard_bins <= train_bins <= %d (got %d, %d)", who, kCfarMaxTrainBins, guard_bins, train_bins); return MDC_EINVAL; }
    if (train_rows == guard_rows && train_bins == guard_bins) { set_error("%s: the guard (%d, %d) is the whole training window: no training cells", who, guard_rows, guard_bins); return MDC_EINVAL; }
    if (rank_permille < 0 || rank_permille > 1000) { set_error("%s: rank_permille must be in 0..1000 (got %d)", who, rank_permille); return MDC_EINVAL; }
    if (!floor_dev && !ratio_dev) return MDC_OK;
    if (!power_dev) { set_error("%s: null buffer", who); return MDC_EINVAL; }
    const uintptr_t bytes = (uintptr_t)(rows * nfft) * sizeof(float), in0 = (uintptr_t)power_dev;
    for (const float* out : {floor_dev, ratio_dev}) {      // an output that overlaps the input would be read by other tiles after it is written
        const uintptr_t out0 = (uintptr_t)out;
        if (out && out0 < in0 + bytes && in0 < out0 + bytes) { set_error("%s: an output overlaps power_dev", who); return MDC_EINVAL; }
    }
    int rc = iq_aligned(who, "power_dev", power_dev, 4);
    if (rc != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "floor_dev", floor_dev, 4)) != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "ratio_dev", ratio_dev, 4)) != MDC_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const int nr = (int)rows, tiles_c = nfft / kCfarTileCols, tiles = tiles_c * ((nr + kCfarTileRows - 1) / kCfarTileRows);
    const size_t lds = (size_t)(kCfarTileRows + 2 * train_rows) * (kCfarTileCols + 2 * train_bins) * sizeof(unsigned);
    return guarded(who, [&]() -> int {
        hipLaunchKernelGGL(iq_cfar_kernel, dim3((unsigned)tiles), dim3(kCfarThreads), lds, s, reinterpret_cast<const unsigned*>(power_dev), nr, nfft, tiles_c,
                           train_rows, train_bins, guard_rows, guard_bins, rank_permille, reinterpret_cast<unsigned*>(floor_dev), ratio_dev);
        MDC_HIP(hipGetLastError());
        return MDC_OK;
    });
}
