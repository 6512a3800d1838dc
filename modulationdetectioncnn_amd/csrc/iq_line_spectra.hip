// mdc_iq_line_spectra -- the line spectra of K stretches of one capture, at up to four orders, in one call, and their float64
// means over the rows; mdc_iq_find_lines -- the line search of S such spectra on the device (include/mdc.h, "batched line
// spectra" and "line search").  Together they turn "one mdc_iq_line_spectrum per (detection, order), a mean and a spectrum
// transfer per order, an argmax and a median on the host" into two calls and one transfer of 48 bytes per spectrum.
//
//   rows      iq_spectrogram_kernel (iq_spectrogram.hip) with the job table, one launch per order into that order's plane of
//             rows_dev: global rows are the jobs' rows back to back (job j owns first_row .. first_row + rows - 1,
//             mdc_iq_line_spectra_rows), and a work-group looks its row's job up and runs the row on the job's slice.  The
//             instructions are the ones a call of mdc_iq_line_spectrum on the slice runs: the bits are that call's by
//             construction.  (One kernel that takes the order at run time would be a second copy of the row's arithmetic, and
//             under the compiler's free choice of where to fuse a multiply and an add two copies need not round alike -- a
//             copy in a device function changed the bits of the nfft = 64 and 128 kernels)
//   means     iq_line_means_kernel: one thread per (job, order index, bin) walks the job's rows top down and adds them in
//             float64 in that fixed order -- acc = 0; acc += (double)row[r][k]; acc / rows, an IEEE division -- so the result is
//             the bits of the sequential numpy loop; adjacent threads are adjacent bins (coalesced), kMeanUnroll loads are in
//             flight per thread, the additions stay in row order.  A job without rows gets 0.0.  It runs after the row kernel
//             on the same stream: no work-group waits for another, there are no atomics.
//   search    iq_find_lines_kernel: one work-group per spectrum.  The spectrum's nfft doubles go into LDS as 64-bit patterns
//             (non-negative finite doubles order as unsigned integers), bins outside the band as all-ones; a bitonic sort in
//             LDS puts the searched values first, ascending, and the two middle order statistics are read off.  The maximum and
//             its smallest bin come from a tree reduction over (pattern, bin) before the sort.  A pattern with the sign bit set
//             (other than -0.0) or an exponent of all ones anywhere in the spectrum makes count -1.
// Launch sizes and every check come from the host copies of the tables; the kernels read the device copies.  The calls only
// enqueue; vector memory for every store.  DESIGN.md 5.23.
#include "mdc_internal.h"

namespace mdc {

namespace {

constexpr int kLineMaxOrders = 4, kLineMinLog2 = 6, kLineMaxLog2 = 12;
constexpr int64_t kLineMaxJobs = (int64_t)1 << 24, kLineMaxRows = (int64_t)1 << 40;
constexpr int kMeanThreads = 256, kMeanUnroll = 8;
constexpr long kMeanGridCap = 4096;
constexpr int kFindThreads = 256;
constexpr long kFindGridCap = 4096;

__global__ __launch_bounds__(kMeanThreads) void iq_line_means_kernel(const float* __restrict__ power, const mdc_iq_line_job* __restrict__ jobs, long njobs,
                                                                    int norders, int nfft, long total_rows, double* __restrict__ mean) {
    const long per_job = (long)norders * nfft, n = njobs * per_job;
    for (long i = (long)blockIdx.x * kMeanThreads + threadIdx.x; i < n; i += (long)gridDim.x * kMeanThreads) {
        const long j = i / per_job, within = i - j * per_job;
        const long o = within / nfft, k = within - o * nfft;
        const long first_row = jobs[j].first_row, rows = jobs[j].rows;
        const float* col = power + (o * total_rows + first_row) * nfft + k;
        double acc = 0.0;
        long r = 0;
        for (; r + kMeanUnroll <= rows; r += kMeanUnroll) {
            float v[kMeanUnroll];
#pragma unroll
            for (int u = 0; u < kMeanUnroll; ++u) v[u] = col[(r + u) * nfft];
#pragma unroll
            for (int u = 0; u < kMeanUnroll; ++u) acc += (double)v[u];
        }
        for (; r < rows; ++r) acc += (double)col[r * nfft];
        mean[i] = rows > 0 ? acc / (double)rows : 0.0;
    }
}

constexpr unsigned long long kOutside = ~0ull;      // a bin outside the band: after every value in the sort

__global__ __launch_bounds__(kFindThreads) void iq_find_lines_kernel(const unsigned long long* __restrict__ spectra, long nspectra, int nfft,
                                                                    const mdc_iq_line_band* __restrict__ bands, mdc_iq_line_record* __restrict__ records) {
    __shared__ unsigned long long key[1 << kLineMaxLog2];
    __shared__ unsigned long long best_v[kFindThreads];
    __shared__ int best_k[kFindThreads];
    __shared__ int cnt[kFindThreads];
    __shared__ int bad;
    const int tid = threadIdx.x, half = nfft / 2;
    for (long s = blockIdx.x; s < nspectra; s += gridDim.x) {
        const unsigned long long* p = spectra + s * nfft;
        const mdc_iq_line_band band = bands[s];
        __syncthreads();      // the previous spectrum's record has been formed from the arrays below
        if (tid == 0) bad = 0;
        __syncthreads();
        unsigned long long bv = 0;
        int bk = -1, c = 0;
        bool b = false;
        for (int k = tid; k < nfft; k += kFindThreads) {      // growing k per thread: the first of equal values stays
            unsigned long long v = p[k];
            if (v == 0x8000000000000000ull) v = 0;            // -0.0 is a zero
            if ((v >> 63) != 0 || ((v >> 52) & 0x7FFull) == 0x7FFull) b = true;
            const double f = (double)(k < half ? k : k - nfft) / (double)nfft, g = band.two_sided && f < 0.0 ? -f : f;
            const bool in = g >= band.lo && g <= band.hi;
            key[k] = in ? v : kOutside;
            if (in) {
                ++c;
                if (bk < 0 || v > bv) { bv = v; bk = k; }
            }
        }
        if (b) bad = 1;      // (every writer writes the same value)
        best_v[tid] = bv;
        best_k[tid] = bk;
        cnt[tid] = c;
        __syncthreads();
        for (int w = kFindThreads / 2; w > 0; w >>= 1) {
            if (tid < w) {
                const unsigned long long ov = best_v[tid + w];
                const int ok = best_k[tid + w];
                if (ok >= 0 && (best_k[tid] < 0 || ov > best_v[tid] || (ov == best_v[tid] && ok < best_k[tid]))) {
                    best_v[tid] = ov;
                    best_k[tid] = ok;
                }
                cnt[tid] += cnt[tid + w];
            }
            __syncthreads();
        }
        for (int k2 = 2; k2 <= nfft; k2 <<= 1) {      // bitonic sort, ascending
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < half; i += kFindThreads) {
                    const int a = ((i & ~(j - 1)) << 1) | (i & (j - 1)), z = a | j;
                    const unsigned long long va = key[a], vz = key[z];
                    const bool up = (a & k2) == 0;
                    if ((va > vz) == up) { key[a] = vz; key[z] = va; }
                }
                __syncthreads();
            }
        }
        if (tid == 0) {
            const int count = cnt[0], k = best_k[0];
            mdc_iq_line_record rec;
            rec.bin = k;
            rec.count = bad ? -1 : count;
            const double* pd = reinterpret_cast<const double*>(p);
            const unsigned long long lo = count > 0 ? key[(count - 1) >> 1] : 0ull, hi = count > 0 ? key[count >> 1] : 0ull;
            rec.peak = k >= 0 ? pd[k] : 0.0;
            rec.left = k >= 0 ? pd[(k + nfft - 1) & (nfft - 1)] : 0.0;
            rec.right = k >= 0 ? pd[(k + 1) & (nfft - 1)] : 0.0;
            rec.median_lo = count > 0 ? __longlong_as_double((long long)lo) : 0.0;
            rec.median_hi = count > 0 ? __longlong_as_double((long long)hi) : 0.0;
            records[s] = rec;
        }
    }
}

// each job's stretch and rows, and their running sum; fills first_row / rows when `fill`, else holds the table to them
int64_t line_jobs_walk(const char* who, mdc_iq_line_job* fill, const mdc_iq_line_job* jobs, int64_t njobs, int64_t pairs_in, int nfft, int64_t hop, int avg) {
    if (njobs < 0 || njobs > kLineMaxJobs) { set_error("%s: njobs must be in 0..%lld (got %lld)", who, (long long)kLineMaxJobs, (long long)njobs); return MDC_EINVAL; }
    if (njobs > 0 && !jobs) { set_error("%s: null jobs", who); return MDC_EINVAL; }
    if (pairs_in < 0 || pairs_in > ((int64_t)1 << 58)) { set_error("%s: pairs_in must be in 0..2^58", who); return MDC_EINVAL; }
    int64_t at = 0;
    for (int64_t j = 0; j < njobs; ++j) {
        const mdc_iq_line_job& b = jobs[j];
        if (b.first_pair < 0 || b.pairs < 0 || b.first_pair > pairs_in || b.pairs > pairs_in - b.first_pair) {
            set_error("%s: job %lld: the stretch [%lld, %lld + %lld) does not lie inside the capture's %lld pairs", who, (long long)j, (long long)b.first_pair,
                      (long long)b.first_pair, (long long)b.pairs, (long long)pairs_in);
            return MDC_EINVAL;
        }
        const int64_t rows = iq_spec_rows(b.pairs, nfft, hop, avg);
        if (fill) {
            fill[j].first_row = at;
            fill[j].rows = rows;
        } else if (b.first_row != at || b.rows != rows) {
            set_error("%s: job %lld: first_row / rows are %lld / %lld, mdc_iq_line_spectra_rows gives %lld / %lld", who, (long long)j, (long long)b.first_row,
                      (long long)b.rows, (long long)at, (long long)rows);
            return MDC_EINVAL;
        }
        at += rows;
        if (at > kLineMaxRows) { set_error("%s: job %lld: more than 2^40 rows in one call", who, (long long)j); return MDC_EINVAL; }
    }
    return at;
}

}  // namespace

}  // namespace mdc

using namespace mdc;

int64_t mdc_iq_line_spectra_rows(mdc_iq_line_job* jobs_host, int64_t njobs, int64_t pairs_in, int nfft, int64_t hop, int avg) {
    static const char who[] = "mdc_iq_line_spectra_rows";
    const int rc = iq_spec_shape_check(who, 0, nfft, hop, avg);
    if (rc != MDC_OK) return (int64_t)rc;
    return line_jobs_walk(who, jobs_host, jobs_host, njobs, pairs_in, nfft, hop, avg);
}

int mdc_iq_line_spectra(const void* iq_dev, int format, int64_t pairs_in, const mdc_iq_line_job* jobs_host, const mdc_iq_line_job* jobs_dev, int64_t njobs,
                        const int* orders_host, int norders, int nfft, int64_t hop, int avg, const int16_t* window_dev, float scale, float* rows_dev,
                        int64_t total_rows, double* mean_dev, void* hip_stream) {
    static const char who[] = "mdc_iq_line_spectra";
    int rc = iq_format_known(who, format);
    if (rc != MDC_OK) return rc;
    if (norders < 1 || norders > kLineMaxOrders) { set_error("%s: norders must be in 1..%d (got %d)", who, kLineMaxOrders, norders); return MDC_EINVAL; }
    if (!orders_host) { set_error("%s: null orders", who); return MDC_EINVAL; }
    int orders[kLineMaxOrders] = {0, 0, 0, 0};
    for (int i = 0; i < norders; ++i) {
        const int o = orders_host[i];
        if (o != 0 && o != 1 && o != 2 && o != 4) { set_error("%s: order %d must be 0 (envelope), 1, 2 or 4 (got %d)", who, i, o); return MDC_EINVAL; }
        for (int k = 0; k < i; ++k)
            if (orders[k] == o) { set_error("%s: order %d appears twice (at %d and %d)", who, o, k, i); return MDC_EINVAL; }
        orders[i] = o;
    }
    if ((rc = iq_spec_shape_check(who, 0, nfft, hop, avg)) != MDC_OK) return rc;
    if (!(scale > 0.f) || !(scale <= 3.402823466e38f)) { set_error("%s: scale must be finite and > 0 (got %g)", who, (double)scale); return MDC_EINVAL; }
    const int64_t total = line_jobs_walk(who, nullptr, jobs_host, njobs, pairs_in, nfft, hop, avg);
    if (total < 0) return (int)total;
    if (total_rows != total) {
        set_error("%s: total_rows is %lld, mdc_iq_line_spectra_rows gives %lld", who, (long long)total_rows, (long long)total);
        return MDC_EINVAL;
    }
    if ((rc = iq_pair_aligned(who, "iq_dev", format, iq_dev)) != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "window_dev", window_dev, 2)) != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "rows_dev", rows_dev, 4)) != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "mean_dev", mean_dev, 8)) != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "jobs_dev", jobs_dev, 8)) != MDC_OK) return rc;
    if (njobs == 0) return MDC_OK;
    if (!jobs_dev || !mean_dev) { set_error("%s: null buffer", who); return MDC_EINVAL; }
    if (total > 0 && (!iq_dev || !window_dev || !rows_dev)) { set_error("%s: null buffer", who); return MDC_EINVAL; }
    const float gain = (float)((double)scale / (double)avg);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return guarded(who, [&]() -> int {
        for (int i = 0; i < norders && total > 0; ++i) {
            const int r = iq_spec_jobs_launch(iq_dev, format, orders[i], nfft, hop, avg, window_dev, gain, rows_dev + (int64_t)i * total * nfft, total, jobs_dev, njobs, s);
            if (r != MDC_OK) return r;
        }
        const long n = (long)njobs * norders * nfft, blocks = (n + kMeanThreads - 1) / kMeanThreads;
        hipLaunchKernelGGL(iq_line_means_kernel, dim3((unsigned)(blocks < kMeanGridCap ? blocks : kMeanGridCap)), dim3(kMeanThreads), 0, s, rows_dev, jobs_dev,
                           (long)njobs, norders, nfft, (long)total, mean_dev);
        MDC_HIP(hipGetLastError());
        return MDC_OK;
    });
}

int mdc_iq_find_lines(const double* spectra_dev, int64_t nspectra, int nfft, const mdc_iq_line_band* bands_host, const mdc_iq_line_band* bands_dev,
                      mdc_iq_line_record* records_dev, void* hip_stream) {
    static const char who[] = "mdc_iq_find_lines";
    if (nfft < (1 << kLineMinLog2) || nfft > (1 << kLineMaxLog2) || (nfft & (nfft - 1)) != 0) {
        set_error("%s: nfft must be a power of two in %d..%d (got %d)", who, 1 << kLineMinLog2, 1 << kLineMaxLog2, nfft);
        return MDC_EINVAL;
    }
    if (nspectra < 0 || nspectra > kLineMaxJobs * kLineMaxOrders) {
        set_error("%s: nspectra must be in 0..%lld (got %lld)", who, (long long)(kLineMaxJobs * kLineMaxOrders), (long long)nspectra);
        return MDC_EINVAL;
    }
    if (nspectra > 0 && !bands_host) { set_error("%s: null bands", who); return MDC_EINVAL; }
    for (int64_t s = 0; s < nspectra; ++s) {
        const mdc_iq_line_band& b = bands_host[s];
        if (b.reserved != 0) { set_error("%s: spectrum %lld: reserved must be 0 (got %d)", who, (long long)s, b.reserved); return MDC_EINVAL; }
        bool any = false;
        for (int k = 0; k < nfft && !any; ++k) {
            const double f = (double)(k < nfft / 2 ? k : k - nfft) / (double)nfft, g = b.two_sided && f < 0.0 ? -f : f;
            any = g >= b.lo && g <= b.hi;
        }
        if (!any) {
            set_error("%s: spectrum %lld: no bin of the %d lies in the band %g .. %g cycles per sample", who, (long long)s, nfft, b.lo, b.hi);
            return MDC_EINVAL;
        }
    }
    if ((reinterpret_cast<uintptr_t>(spectra_dev) & 7) != 0 || (reinterpret_cast<uintptr_t>(bands_dev) & 7) != 0 ||
        (reinterpret_cast<uintptr_t>(records_dev) & 7) != 0) {
        set_error("%s: spectra_dev, bands_dev and records_dev must be 8-byte aligned", who);
        return MDC_EINVAL;
    }
    if (nspectra == 0) return MDC_OK;
    if (!spectra_dev || !bands_dev || !records_dev) { set_error("%s: null buffer", who); return MDC_EINVAL; }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    return guarded(who, [&]() -> int {
        hipLaunchKernelGGL(iq_find_lines_kernel, dim3((unsigned)(nspectra < kFindGridCap ? nspectra : kFindGridCap)), dim3(kFindThreads), 0, st,
                           reinterpret_cast<const unsigned long long*>(spectra_dev), (long)nspectra, nfft, bands_dev, records_dev);
        MDC_HIP(hipGetLastError());
        return MDC_OK;
    });
}
