// mdc_iq_spectrogram_components -- threshold a (rows x nfft) float32 spectrogram cell by cell, join the on-cells into connected
// components under a rectangular reach, number them by their first cell and reduce each to a box, a cell count and a peak
// (include/mdc.h, "spectrogram components"; the Python restatement is tests/iq_components_ref.py).
//
// Everything works on CENTRED cell indices i = r * nfft + c, c = (k + nfft/2) mod nfft = k ^ (nfft/2): cell i lives at position
// i ^ (nfft/2) of power_dev and labels_dev.  labels_dev doubles as the union-find forest until the last kernel: an on-cell holds
// the index of a cell of its component that is not larger than its own ("parent"; a root holds itself), an off cell -1.  Links
// only ever go to smaller indices, so a tree's root is its smallest cell and the root of a finished component is the cell the
// header numbers it by.  Seven launches on the stream, none waits for another work-group (a kernel boundary is what makes one
// phase's stores visible to the next on every XCD):
//   1 tile      a work-group thresholds a tile of kTileRows x kTileCols cells into LDS, unites the on-cells of the tile there
//               (LDS atomicMin union-find on local indices, which order like the global ones), and writes every on-cell's tile root.
//   2 border    the on-cells within reach of a tile's right, left or lower edge unite with their forward neighbours in OTHER tiles:
//               a global union-find on labels_dev, every access an agent-scope atomic.
//   3 flatten   a chunk of kChunk consecutive indices per work-group: every on-cell walks to its root and stores it; the roots of
//               the chunk (label == own index) are counted into work_dev[chunk].
//   4 scan      one work-group turns the counts into exclusive offsets in place; the total is *count_dev.
//   5 rank      per chunk again: a root's number is offset + its rank among the chunk's roots; it initialises its record and
//               leaves -2 - number in its own cell.
//   6 reduce    every on-cell reads its root's cell (encoded or already final: both decode to the number), stores the number as
//               its final label and folds row, column, count and peak key into the record -- aggregated per wave first (a wave is
//               64 consecutive cells of one row), then integer atomicMin / atomicMax / atomicAdd and one 64-bit atomicMax.  (Reading
//               the record first to leave out atomics that cannot move a field was measured slower: DESIGN.md 5.21.)
//   7 records   the packed key (pattern << 32 | ~index, kept in the record's last 8 bytes) becomes peak, peak_row, peak_bin.
// Link search: with reach (a, b) an on-cell looks at its forward half, b cells to the right and a rows of 2b + 1 below.  In its
// own row the NEAREST on-cell suffices (that one links on); in a row below, an on-cell whose predecessor in the window is at most b
// away is already linked to that predecessor by the row rule, so at most two unions per row remain: <= 1 + 2a = 9 per cell.
// Loop bounds are stated at the loops.  Nothing is summed in floating point; the atomics are integer min / max / add and the
// key's max, whose results do not depend on arrival order: the same bits on every run.  All stores are vector stores from plain
// C++.  workspace: one 32-bit counter per chunk.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; no kernel spills, no scratch):
//   kernel                 VGPR  SGPR  LDS bytes  threads
//   iq_comp_tile_kernel       28    71       8192      256
//   iq_comp_border_kernel     16    50          0      256
//   iq_comp_flatten_kernel    10    25          4      256
//   iq_comp_scan_kernel       34    61         68     1024
//   iq_comp_rank_kernel       18    38         64      256
//   iq_comp_reduce_kernel     24    32          0      256
//   iq_comp_records_kernel     6    16          0      256
#include "mdc_internal.h"

namespace mdc {

namespace {

constexpr int kCompMinLog2 = 6, kCompMaxLog2 = 12, kCompMaxReach = 4;
constexpr int kTileRows = 32, kTileCols = 64, kTileCells = kTileRows * kTileCols;      // kTileCols divides every nfft
constexpr int kCompThreads = 256, kTilePerThread = kTileCells / kCompThreads;
constexpr int kChunk = 1024, kChunkPerThread = kChunk / kCompThreads;                 // a wave's 64 cells share a row (64 | nfft)
constexpr int kScanThreads = 1024;
static_assert(kTileCols == 64, "a wave is one tile row");

#define MDC_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define MDC_RLX_GROUP __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

// ---- union-find on the tile in LDS (indices: lr * kTileCols + lc) ---------------------------------------------------------------
// bound: lab[v] <= v always (a cell starts at itself and atomicMin only lowers it), so the walk visits strictly decreasing
// indices and ends, after at most v steps, at a cell that holds itself.
__device__ __forceinline__ int tile_find(int* lab, int v) {
    for (;;) {
        const int p = __hip_atomic_load(&lab[v], MDC_RLX_GROUP);
        if (p == v) return v;
        v = p;
    }
}

// bound: every retry continues from what the failed atomicMin returned, old < x, and y < x: max(x, y) strictly decreases, so
// there are at most max(x, y) rounds and no livelock.  Nothing is lost: when lab[x] drops from old to y the pair (old, y) is
// what the loop goes on to unite.
__device__ __forceinline__ void tile_unite(int* lab, int x, int y) {
    x = tile_find(lab, x);
    y = tile_find(lab, y);
    while (x != y) {
        if (x < y) { const int t = x; x = y; y = t; }
        const int old = __hip_atomic_fetch_min(&lab[x], y, MDC_RLX_GROUP);
        if (old == x) break;      // x was a root and now hangs under y
        x = tile_find(lab, old);
    }
}

// ---- the same on labels_dev (indices: centred cell indices; cell i lives at i ^ half) -------------------------------------------
__device__ __forceinline__ int cell_load(int* labels, int half, int i) { return __hip_atomic_load(&labels[i ^ half], MDC_RLX_AGENT); }

// bound: as tile_find -- a label is never larger than its cell's index and only ever decreases; a stale value is an older
// parent, still a cell of the same component with a smaller index.
__device__ __forceinline__ int cell_find(int* labels, int half, int v) {
    for (;;) {
        const int p = cell_load(labels, half, v);
        if (p == v) return v;
        v = p;
    }
}

// bound: as tile_unite.  The atomicMin is the one access that must be exact, and it is a read-modify-write at agent scope; a find
// that ended on a stale root is caught by the value the atomicMin returns.
__device__ __forceinline__ void cell_unite(int* labels, int half, int x, int y) {
    x = cell_find(labels, half, x);
    y = cell_find(labels, half, y);
    while (x != y) {
        if (x < y) { const int t = x; x = y; y = t; }
        const int old = __hip_atomic_fetch_min(&labels[x ^ half], y, MDC_RLX_AGENT);
        if (old == x) break;
        x = cell_find(labels, half, old);
    }
}

// ---- 1: threshold and label one tile ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCompThreads) void iq_comp_tile_kernel(const float* __restrict__ power, const float* __restrict__ thresh, int rows, int nfft,
                                                                   int tiles_c, int reach_r, int reach_c, int* __restrict__ labels) {
    __shared__ int lab[kTileCells];
    const int tid = threadIdx.x, half = nfft >> 1;
    const int r0 = (int)(blockIdx.x / (unsigned)tiles_c) * kTileRows, c0 = (int)(blockIdx.x % (unsigned)tiles_c) * kTileCols;
    unsigned mine = 0;      // bit j: my j-th cell is on
#pragma unroll
    for (int j = 0; j < kTilePerThread; ++j) {
        const int l = j * kCompThreads + tid, r = r0 + (l >> 6), k = (c0 + (l & 63)) ^ half;
        bool on = false;
        if (r < rows) on = power[r * nfft + k] > thresh[k];      // f32 compare: equality, NaN and a +Inf threshold are off
        mine |= (unsigned)on << j;
        lab[l] = on ? l : -1;
    }
    __syncthreads();
    for (int j = 0; j < kTilePerThread; ++j) {      // bound: 8 cells per thread
        if (!((mine >> j) & 1u)) continue;
        const int l = j * kCompThreads + tid, lr = l >> 6, lc = l & 63;
        for (int dc = 1; dc <= reach_c && lc + dc < kTileCols; ++dc)      // bound: reach_c <= 4; the nearest on-cell to the right
            if (__hip_atomic_load(&lab[l + dc], MDC_RLX_GROUP) >= 0) { tile_unite(lab, l, l + dc); break; }
        for (int dr = 1; dr <= reach_r && lr + dr < kTileRows; ++dr) {      // bound: reach_r <= 4 rows below
            int prev = -16;      // dc of the last on-cell seen in this row's window
            for (int dc = -reach_c; dc <= reach_c; ++dc) {      // bound: 2 reach_c + 1 <= 9 cells
                const int cc = lc + dc;
                if (cc < 0 || cc >= kTileCols) continue;
                const int n = l + dr * kTileCols + dc;
                if (__hip_atomic_load(&lab[n], MDC_RLX_GROUP) < 0) continue;
                if (dc - prev > reach_c) tile_unite(lab, l, n);      // (else the row rule has linked it to its predecessor)
                prev = dc;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kTilePerThread; ++j) {
        const int l = j * kCompThreads + tid, r = r0 + (l >> 6), k = (c0 + (l & 63)) ^ half;
        if (r >= rows) continue;
        int g = -1;
        if ((mine >> j) & 1u) {
            const int root = tile_find(lab, l);
            g = (r0 + (root >> 6)) * nfft + c0 + (root & 63);
        }
        labels[r * nfft + k] = g;
    }
}

// ---- 2: unite across tile borders ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCompThreads) void iq_comp_border_kernel(int rows, int nfft, int tiles_c, int reach_r, int reach_c, int* labels) {
    const int tid = threadIdx.x, half = nfft >> 1;
    const int trow = (int)(blockIdx.x / (unsigned)tiles_c), tcol = (int)(blockIdx.x % (unsigned)tiles_c);
    const int r0 = trow * kTileRows, c0 = tcol * kTileCols;
    for (int j = 0; j < kTilePerThread; ++j) {      // bound: 8 cells per thread
        const int l = j * kCompThreads + tid, lr = l >> 6, lc = l & 63, r = r0 + lr, c = c0 + lc;
        const bool side = lc + reach_c >= kTileCols || lc < reach_c, below = lr + reach_r >= kTileRows;
        if (r >= rows || !(below || side)) continue;      // its whole forward half lies in its own tile
        const int i = r * nfft + c;
        if (cell_load(labels, half, i) < 0) continue;
        for (int dc = 1; dc <= reach_c && c + dc < nfft; ++dc)      // bound: reach_c <= 4; the nearest on-cell to the right
            if (cell_load(labels, half, i + dc) >= 0) {
                if (lc + dc >= kTileCols) cell_unite(labels, half, i, i + dc);      // (in the tile: kernel 1 has united them)
                break;
            }
        for (int dr = 1; dr <= reach_r && r + dr < rows; ++dr) {      // bound: reach_r <= 4 rows below
            const bool other_row = lr + dr >= kTileRows;
            if (!other_row && !side) continue;
            int prev = -16;
            for (int dc = -reach_c; dc <= reach_c; ++dc) {      // bound: 2 reach_c + 1 <= 9 cells
                const int cc = c + dc;
                if (cc < 0 || cc >= nfft) continue;      // the band is not circular
                const int n = i + dr * nfft + dc;
                if (cell_load(labels, half, n) < 0) continue;
                if (dc - prev > reach_c && (other_row || lc + dc < 0 || lc + dc >= kTileCols)) cell_unite(labels, half, i, n);
                prev = dc;
            }
        }
    }
}

// ---- 3: every cell to its root; roots per chunk ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCompThreads) void iq_comp_flatten_kernel(int cells, int nfft, int* labels, unsigned* __restrict__ counts) {
    __shared__ unsigned total;
    const int tid = threadIdx.x, half = nfft >> 1;
    if (tid == 0) total = 0u;
    __syncthreads();
    unsigned roots = 0;
#pragma unroll
    for (int j = 0; j < kChunkPerThread; ++j) {
        const long i64 = (long)blockIdx.x * kChunk + j * kCompThreads + tid;
        if (i64 >= cells) continue;
        const int i = (int)i64, v = cell_load(labels, half, i);
        if (v < 0) continue;
        if (v == i) { ++roots; continue; }
        const int root = cell_find(labels, half, v);
        if (root != v) __hip_atomic_store(&labels[i ^ half], root, MDC_RLX_AGENT);      // (a reader sees v or root: both lead to root)
    }
    if (roots) atomicAdd(&total, roots);      // an integer sum: the order does not matter
    __syncthreads();
    if (tid == 0) counts[blockIdx.x] = total;
}

// ---- 4: exclusive scan of the chunk counts, in place; the total ---------------------------------------------------------------------
__global__ __launch_bounds__(kScanThreads) void iq_comp_scan_kernel(unsigned* __restrict__ counts, int nchunks, long long* __restrict__ count_out) {
    __shared__ unsigned wsum[kScanThreads / 64];
    __shared__ unsigned carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry = 0u;
    __syncthreads();
    for (int base = 0; base < nchunks; base += kScanThreads) {      // bound: ceil(nchunks / 1024) rounds
        const int j = base + tid;
        const unsigned v = j < nchunks ? counts[j] : 0u;
        unsigned incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {      // bound: 6 steps
            const unsigned up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned before = carry, all = 0u;
#pragma unroll
        for (int w = 0; w < kScanThreads / 64; ++w) {      // bound: 16 waves
            if (w < wave) before += wsum[w];
            all += wsum[w];
        }
        if (j < nchunks) counts[j] = before + incl - v;
        __syncthreads();
        if (tid == 0) carry += all;
        __syncthreads();
    }
    if (tid == 0) *count_out = (long long)carry;
}

// ---- 5: number the roots, initialise their records ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kCompThreads) void iq_comp_rank_kernel(int cells, int nfft, int* labels, const unsigned* __restrict__ offsets,
                                                                   mdc_iq_component* __restrict__ comps, long long capacity) {
    __shared__ unsigned wcount[kChunkPerThread][kCompThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = nfft >> 1;
    bool root[kChunkPerThread];
    unsigned long long ballot[kChunkPerThread];
#pragma unroll
    for (int j = 0; j < kChunkPerThread; ++j) {
        const long i64 = (long)blockIdx.x * kChunk + j * kCompThreads + tid;
        root[j] = i64 < cells && labels[(int)i64 ^ half] == (int)i64;
        ballot[j] = __ballot(root[j]);
        if (lane == 0) wcount[j][wave] = (unsigned)__popcll(ballot[j]);
    }
    __syncthreads();
    const unsigned first = offsets[blockIdx.x];
#pragma unroll
    for (int j = 0; j < kChunkPerThread; ++j) {
        if (!root[j]) continue;
        unsigned before = first + (unsigned)__popcll(ballot[j] & ((1ull << lane) - 1ull));
        for (int q = 0; q < j * (kCompThreads / 64) + wave; ++q) before += (&wcount[0][0])[q];      // bound: < 16 earlier waves of the chunk
        const int i = blockIdx.x * kChunk + j * kCompThreads + tid;
        labels[i ^ half] = -2 - (int)before;      // decoded by kernel 6
        if ((long long)before < capacity) {
            mdc_iq_component rec;
            rec.row_first = 2147483647; rec.row_stop = 0; rec.bin_first = 2147483647; rec.bin_stop = 0;
            rec.cells = 0; rec.peak = 0.0f; rec.peak_row = 0; rec.peak_bin = 0;      // (the last 8 bytes: the key, 0 loses to every cell's)
            comps[before] = rec;
        }
    }
}

// ---- 6: final labels, boxes, counts, peak keys ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCompThreads) void iq_comp_reduce_kernel(const float* __restrict__ power, int cells, int nfft, int lognfft, int* labels,
                                                                     mdc_iq_component* comps, long long capacity) {
    const int tid = threadIdx.x, lane = tid & 63, half = nfft >> 1;
    for (int j = 0; j < kChunkPerThread; ++j) {      // bound: 4 cells per thread; no lane leaves before the wave's shuffles are done
        const long i64 = (long)blockIdx.x * kChunk + j * kCompThreads + tid;
        const int i = (int)i64;
        int slot = -1;
        unsigned long long key = 0ull;
        if (i64 < cells) {
            const int v = cell_load(labels, half, i);
            if (v <= -2) slot = -2 - v;      // a root, numbered by kernel 5
            else if (v >= 0) {               // its root's cell: -2 - number, or the number itself once the root's own thread has been here
                const int e = cell_load(labels, half, v);
                slot = e <= -2 ? -2 - e : e;
            }
            if (slot >= 0) {
                __hip_atomic_store(&labels[i ^ half], slot, MDC_RLX_AGENT);
                key = ((unsigned long long)__float_as_uint(power[i ^ half]) << 32) | (unsigned)~(unsigned)i;
            }
        }
        bool pending = slot >= 0 && (long long)slot < capacity;
        const int row = (int)((i64 - lane) >> lognfft), col0 = (int)((i64 - lane) & (nfft - 1));      // the wave's 64 cells: one row, columns col0 ..
        for (;;) {      // bound: every round retires at least the leading lane: <= 64 rounds
            const unsigned long long open = __ballot(pending);
            if (!open) break;
            const int lead = __ffsll((long long)open) - 1;
            const int s = __shfl(slot, lead);
            const bool in = pending && slot == s;
            const unsigned long long who = __ballot(in);
            unsigned hi = in ? (unsigned)(key >> 32) : 0u, lo = in ? (unsigned)key : 0u;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {      // bound: 6 steps; the largest key of the lanes that are in
                const unsigned ohi = __shfl_xor(hi, d), olo = __shfl_xor(lo, d);
                if (ohi > hi || (ohi == hi && olo > lo)) { hi = ohi; lo = olo; }
            }
            if (lane == lead) {
                mdc_iq_component* rec = comps + s;
                const int cmin = col0 + __ffsll((long long)who) - 1, cmax = col0 + 63 - __clzll((long long)who);
                atomicMin(&rec->row_first, row);
                atomicMax(&rec->row_stop, row + 1);
                atomicMin(&rec->bin_first, cmin);
                atomicMax(&rec->bin_stop, cmax + 1);
                atomicAdd(&rec->cells, (int)__popcll(who));
                atomicMax(reinterpret_cast<unsigned long long*>(&rec->peak_row), ((unsigned long long)hi << 32) | lo);
            }
            if (in) pending = false;
        }
    }
}

// ---- 7: unpack the peak keys ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCompThreads) void iq_comp_records_kernel(mdc_iq_component* __restrict__ comps, long long capacity, const long long* __restrict__ count,
                                                                      int nfft, int lognfft) {
    const long long n = *count < capacity ? *count : capacity;
    const long long i = (long long)blockIdx.x * kCompThreads + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = *reinterpret_cast<const unsigned long long*>(&comps[i].peak_row);
    const unsigned at = ~(unsigned)key;
    comps[i].peak = __uint_as_float((unsigned)(key >> 32));
    comps[i].peak_row = (int)(at >> lognfft);
    comps[i].peak_bin = (int)(at & (unsigned)(nfft - 1));
}

}  // namespace

}  // namespace mdc

using namespace mdc;

static_assert(sizeof(mdc_iq_component) == 32, "mdc_iq_component is 32 bytes");

int64_t mdc_iq_spectrogram_components_workspace(int64_t rows, int nfft) {
    const char* who = "mdc_iq_spectrogram_components_workspace";
    if (pow2_log2(nfft, kCompMinLog2, kCompMaxLog2) < 0) { set_error("%s: nfft must be a power of two in %d..%d (got %d)", who, 1 << kCompMinLog2, 1 << kCompMaxLog2, nfft); return MDC_EINVAL; }
    if (rows < 1 || rows > 2147483647LL / nfft) { set_error("%s: rows must be >= 1 and rows * nfft <= 2^31-1 (got %lld)", who, (long long)rows); return MDC_EINVAL; }
    const int64_t nchunks = (rows * nfft + kChunk - 1) / kChunk;
    return (nchunks * 4 + 15) / 16 * 16;
}

int mdc_iq_spectrogram_components(const float* power_dev, int64_t rows, int nfft, const float* thresh_dev, int reach_rows, int reach_bins,
                                  int32_t* labels_dev, mdc_iq_component* comps_dev, int64_t capacity, int64_t* count_dev, void* work_dev,
                                  void* hip_stream) {
    const char* who = "mdc_iq_spectrogram_components";
    const int lognfft = pow2_log2(nfft, kCompMinLog2, kCompMaxLog2);
    if (lognfft < 0) { set_error("%s: nfft must be a power of two in %d..%d (got %d)", who, 1 << kCompMinLog2, 1 << kCompMaxLog2, nfft); return MDC_EINVAL; }
    if (rows < 1 || rows > 2147483647LL / nfft) { set_error("%s: rows must be >= 1 and rows * nfft <= 2^31-1 (got %lld)", who, (long long)rows); return MDC_EINVAL; }
    if (reach_rows < 0 || reach_rows > kCompMaxReach) { set_error("%s: reach_rows must be in 0..%d (got %d)", who, kCompMaxReach, reach_rows); return MDC_EINVAL; }
    if (reach_bins < 0 || reach_bins > kCompMaxReach) { set_error("%s: reach_bins must be in 0..%d (got %d)", who, kCompMaxReach, reach_bins); return MDC_EINVAL; }
    if (capacity < 0) { set_error("%s: capacity must be >= 0 (got %lld)", who, (long long)capacity); return MDC_EINVAL; }
    if (!power_dev || !thresh_dev || !labels_dev || !count_dev || !work_dev || (capacity > 0 && !comps_dev)) { set_error("%s: null buffer", who); return MDC_EINVAL; }
    int rc = iq_aligned(who, "power_dev", power_dev, 4);
    if (rc != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "thresh_dev", thresh_dev, 4)) != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "labels_dev", labels_dev, 4)) != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "comps_dev", comps_dev, 8)) != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "count_dev", count_dev, 8)) != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "work_dev", work_dev, 16)) != MDC_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const int cells = (int)(rows * nfft), nr = (int)rows;
    const int tiles_c = nfft / kTileCols, tiles = tiles_c * ((nr + kTileRows - 1) / kTileRows), nchunks = (int)(((int64_t)cells + kChunk - 1) / kChunk);
    unsigned* counts = static_cast<unsigned*>(work_dev);
    long long* count = reinterpret_cast<long long*>(count_dev);
    const long long cap = (long long)capacity;
    return guarded(who, [&]() -> int {
        hipLaunchKernelGGL(iq_comp_tile_kernel, dim3((unsigned)tiles), dim3(kCompThreads), 0, s, power_dev, thresh_dev, nr, nfft, tiles_c, reach_rows,
                           reach_bins, labels_dev);
        MDC_HIP(hipGetLastError());
        if (reach_rows > 0 || reach_bins > 0) {      // reach (0, 0): every on-cell is its own component already
            hipLaunchKernelGGL(iq_comp_border_kernel, dim3((unsigned)tiles), dim3(kCompThreads), 0, s, nr, nfft, tiles_c, reach_rows, reach_bins, labels_dev);
            MDC_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(iq_comp_flatten_kernel, dim3((unsigned)nchunks), dim3(kCompThreads), 0, s, cells, nfft, labels_dev, counts);
        MDC_HIP(hipGetLastError());
        hipLaunchKernelGGL(iq_comp_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, counts, nchunks, count);
        MDC_HIP(hipGetLastError());
        hipLaunchKernelGGL(iq_comp_rank_kernel, dim3((unsigned)nchunks), dim3(kCompThreads), 0, s, cells, nfft, labels_dev, counts, comps_dev, cap);
        MDC_HIP(hipGetLastError());
        hipLaunchKernelGGL(iq_comp_reduce_kernel, dim3((unsigned)nchunks), dim3(kCompThreads), 0, s, power_dev, cells, nfft, lognfft, labels_dev, comps_dev, cap);
        MDC_HIP(hipGetLastError());
        if (cap > 0) {
            const long long most = cap < (long long)cells ? cap : (long long)cells;      // there are never more components than cells
            hipLaunchKernelGGL(iq_comp_records_kernel, dim3((unsigned)((most + kCompThreads - 1) / kCompThreads)), dim3(kCompThreads), 0, s, comps_dev, cap, count,
                               nfft, lognfft);
            MDC_HIP(hipGetLastError());
        }
        return MDC_OK;
    });
}
