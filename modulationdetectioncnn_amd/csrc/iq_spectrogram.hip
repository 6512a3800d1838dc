// mdc_iq_spectrogram -- the power spectrogram of an integer I/Q capture on the device (include/mdc.h, "power spectrogram"; the
// float64 numpy restatement is tests/iq_spectrum_ref.py).  One work-group owns a row: it transforms the row's `avg` segments one
// after the other, sums |X|^2 in registers in that fixed order and stores the row once -- the same inputs give the same bits on
// every run, and a row's bits do not depend on what else the call computes.  Work-groups stride over the rows (grid cap
// kSpecGridCap).
//
//   threads   T = nfft / 4 clamped to 64..512: one radix-4 butterfly per thread and pass up to nfft = 2048, two at 4096 (measured:
//             512 threads with two each take 0.85 of the time of 256 with four); at nfft = 64 a single wave with
//             16 busy lanes.
//   stage     each thread takes four adjacent pairs at a time (iq_mix.h's load_quad: one 8- or 16-byte vector load, widened to
//             16-bit full scale), multiplies them by the window's int16 values in int32 (exact, |v| < 2^30), converts to f32 and
//             writes four complex values into the LDS image.
//   transform iq_fft.h: every pass but the last in place in the LDS image; the last pass's outputs stay in registers, and the
//             thread adds their squared magnitudes to its accumulators, bins t + k nfft/4 (t + k nfft/2 after an odd log2's
//             radix-2 pass).  The row's store is then coalesced.
//   LDS       the image (iq_fft.h: one element of padding after every 16) and the three twiddle tables.  nfft = 4096: 34 KiB of
//             image + 24 KiB of twiddles, two work-groups per CU.
// mdc_iq_line_spectrum is the same kernel with ORDER != 1: the staging alone differs (spec_stage; include/mdc.h, "line spectrum";
// tests/iq_line_ref.py), everything from the image on is shared -- DESIGN.md 5.19.
// mdc_iq_line_spectra (iq_line_spectra.hip) is the same kernel again, handed a JOB TABLE: its rows are then the jobs' rows back to
// back, and a work-group looks its row's job up (a binary search of the table's first_row column, uniform over the work-group)
// and runs the row on the job's slice -- base pointer iq + first_pair, bound `pairs`, the row counted from the job's first.  The
// very instructions that serve a call on the slice compute the row, so its bits are that call's by construction, and no pair
// outside the job is read: every segment of a row the rows function counts lies inside the bound.
// The call only enqueues; vector memory for every store.
#include "iq_fft.h"
#include "iq_mix.h"

namespace mdc {

namespace {

constexpr int kSpecMinLog2 = 6, kSpecMaxLog2 = 12, kSpecMaxAvg = 4096;
constexpr long kSpecGridCap = 2048;      // work-groups; beyond it the kernel strides (_cabi.SPECTROGRAM_GRID_CAP)

__host__ __device__ constexpr int spec_threads(int log2n) { return (1 << log2n) / 4 < 64 ? 64 : (1 << log2n) / 4 > 512 ? 512 : (1 << log2n) / 4; }
__device__ __forceinline__ float norm2(float2 a) { return a.x * a.x + a.y * a.y; }

// What is transformed (ORDER; include/mdc.h, "line spectrum"): the widened pair itself (1: mdc_iq_spectrogram), or an exact
// integer function of it -- its envelope I^2 + Q^2 (0), its square (2) or its fourth power (4) -- times the window's value and
// 2^-q, q = 16 / 0 / 16 / 48.  Orders 0 and 2 stay in 32-bit integers (I^2 + Q^2 <= 2^31 as unsigned; I^2 - Q^2 and I Q within
// +-2^30, the factor 2 of 2 I Q goes into the window's factor); order 4 squares that pair in 64-bit integers (|.| <= 2^62).
// Each value is rounded twice on its way into the image: the integer's conversion to f32, and the product with w 2^-q (itself
// exact: an int16 times a power of two).
template <int ORDER>
__device__ __forceinline__ float2 spec_stage(int I, int Q, int w) {
    if constexpr (ORDER == 1) {
        return make_float2((float)(I * w), (float)(Q * w));
    } else if constexpr (ORDER == 0) {
        return make_float2((float)((unsigned)(I * I) + (unsigned)(Q * Q)) * ((float)w * 0x1p-16f), 0.f);
    } else {
        const int a = I * I - Q * Q, b = I * Q;      // the square is (a, 2b)
        if constexpr (ORDER == 2) {
            return make_float2((float)a * ((float)w * 0x1p-16f), (float)b * ((float)w * 0x1p-15f));
        } else {
            static_assert(ORDER == 4, "orders 0, 1, 2 and 4");
            const long long aa = (long long)a * a, bb = (long long)b * b, ab = (long long)a * b;
            const float ws = (float)w * 0x1p-48f;
            return make_float2((float)(aa - 4 * bb) * ws, (float)(4 * ab) * ws);
        }
    }
}

template <int FMT, int LOG2N, int ORDER>
__global__ __launch_bounds__(spec_threads(LOG2N)) void iq_spectrogram_kernel(const unsigned char* __restrict__ iq, long pairs, long hop, int avg,
                                                                            const short* __restrict__ window, float gain,
                                                                            float* __restrict__ power, long rows,
                                                                            const mdc_iq_line_job* __restrict__ jobs, long njobs) {
    constexpr int N = 1 << LOG2N, NB = N / 4, T = spec_threads(LOG2N);
    constexpr int B = (NB + T - 1) / T;              // radix-4 butterflies (and staged quads) per thread
    constexpr bool kWhole = NB % T == 0;             // false only for nfft 64 and 128: fewer butterflies than lanes
    constexpr int R = fft_last_radix(LOG2N), NL = N / R;      // the last pass: NL butterflies of R outputs
    constexpr int BL = (NL + T - 1) / T;             // of them per thread
    constexpr bool kLastWhole = NL % T == 0;
    __shared__ float2 x[fft_slot(N)];
    __shared__ float2 tw[3 * NB];
    const int tid = threadIdx.x;
    fft_fill_twiddles<LOG2N, T>(tw, tid);

    for (long grow = blockIdx.x; grow < rows; grow += gridDim.x) {
        const unsigned char* src = iq;      // the capture, or with a job table the row's job: all uniform over the work-group
        long bound = pairs, row = grow;
        if (jobs) {
            long lo = 0, hi = njobs - 1;      // the last job whose first_row is <= grow owns the row (jobs without rows share their
            while (lo < hi) {                 // first_row with the owner and come before it)
                const long mid = (lo + hi + 1) >> 1;
                if (jobs[mid].first_row <= grow) lo = mid; else hi = mid - 1;
            }
            src = iq + jobs[lo].first_pair * Quad<FMT>::kPairBytes;
            bound = jobs[lo].pairs;
            row = grow - jobs[lo].first_row;
        }
        float acc[R * BL];
#pragma unroll
        for (int i = 0; i < R * BL; ++i) acc[i] = 0.f;
        for (int sg = 0; sg < avg; ++sg) {
            const long start = (row * avg + sg) * hop;
            __syncthreads();      // the twiddles are in place; the previous segment's last pass has read its image
#pragma unroll
            for (int i = 0; i < B; ++i) {
                const int q = tid + i * T;
                if (kWhole || q < NB) {
                    int I[4], Q[4];
                    load_quad<FMT>(src, start + 4 * q, bound, I, Q);
                    short w[4];
                    __builtin_memcpy(w, window + 4 * q, sizeof(w));
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[fft_slot(4 * q + e)] = spec_stage<ORDER>(I[e], Q[e], (int)w[e]);
                }
            }
            __syncthreads();
            float2 y[B][4];
            fft_stored_passes<LOG2N, B, T>(x, tw, 0, tid, y);
            fft_last_pass<LOG2N, BL, T>(x, 0, tid, [&](int i, int k, int, float2 v) { acc[R * i + k] += norm2(v); });
        }
        float* out = power + grow * N;
#pragma unroll
        for (int i = 0; i < BL; ++i) {
            const int t = tid + i * T;
            if (kLastWhole || t < NL) {
#pragma unroll
                for (int k = 0; k < R; ++k) out[t + k * NL] = acc[R * i + k] * gain;
            }
        }
    }
}

template <int FMT, int LOG2N, int ORDER>
int spec_launch(const unsigned char* iq, int64_t pairs, int64_t hop, int avg, const int16_t* window, float gain, float* power, int64_t rows,
                const mdc_iq_line_job* jobs, int64_t njobs, hipStream_t s) {
    const dim3 g((unsigned)(rows < kSpecGridCap ? rows : kSpecGridCap)), b(spec_threads(LOG2N));
    hipLaunchKernelGGL((iq_spectrogram_kernel<FMT, LOG2N, ORDER>), g, b, 0, s, iq, (long)pairs, (long)hop, avg, reinterpret_cast<const short*>(window), gain, power,
                       (long)rows, jobs, (long)njobs);
    MDC_HIP(hipGetLastError());
    return MDC_OK;
}

int spec_shape_check(const char* who, int64_t pairs, int nfft, int64_t hop, int avg) {
    if (pow2_log2(nfft, kSpecMinLog2, kSpecMaxLog2) < 0) { set_error("%s: nfft must be a power of two in %d..%d (got %d)", who, 1 << kSpecMinLog2, 1 << kSpecMaxLog2, nfft); return MDC_EINVAL; }
    if (hop < 1) { set_error("%s: hop must be >= 1 pair (got %lld)", who, (long long)hop); return MDC_EINVAL; }
    if (avg < 1 || avg > kSpecMaxAvg) { set_error("%s: avg must be in 1..%d (got %d)", who, kSpecMaxAvg, avg); return MDC_EINVAL; }
    if (pairs < 0) { set_error("%s: negative pair count", who); return MDC_EINVAL; }
    return MDC_OK;
}

int64_t spec_rows(int64_t pairs, int nfft, int64_t hop, int avg) {
    return iq_span_count(pairs, nfft, hop) / avg;
}

// format, log2 nfft and order as template arguments; jobs == nullptr: the rows of the capture itself
int spec_dispatch(int format, int order, int log2n, const unsigned char* p, int64_t pairs, int64_t hop, int avg, const int16_t* window, float gain, float* power,
                  int64_t rows, const mdc_iq_line_job* jobs, int64_t njobs, hipStream_t s) {
    return with_format(format, [&](auto fmt) {
        return with_log2<kSpecMinLog2, kSpecMaxLog2>(log2n, [&](auto l2) {
            constexpr int F = decltype(fmt)::value, L = decltype(l2)::value;
            switch (order) {
                case 0: return spec_launch<F, L, 0>(p, pairs, hop, avg, window, gain, power, rows, jobs, njobs, s);
                case 1: return spec_launch<F, L, 1>(p, pairs, hop, avg, window, gain, power, rows, jobs, njobs, s);
                case 2: return spec_launch<F, L, 2>(p, pairs, hop, avg, window, gain, power, rows, jobs, njobs, s);
                default: return spec_launch<F, L, 4>(p, pairs, hop, avg, window, gain, power, rows, jobs, njobs, s);
            }
        });
    });
}

}  // namespace

// what iq_line_spectra.hip needs of this file (mdc_internal.h)
int iq_spec_shape_check(const char* who, int64_t pairs, int nfft, int64_t hop, int avg) { return spec_shape_check(who, pairs, nfft, hop, avg); }
int64_t iq_spec_rows(int64_t pairs, int nfft, int64_t hop, int avg) { return spec_rows(pairs, nfft, hop, avg); }
int iq_spec_jobs_launch(const void* iq, int format, int order, int nfft, int64_t hop, int avg, const int16_t* window, float gain, float* power, int64_t rows,
                        const mdc_iq_line_job* jobs_dev, int64_t njobs, hipStream_t s) {
    return spec_dispatch(format, order, pow2_log2(nfft, kSpecMinLog2, kSpecMaxLog2), static_cast<const unsigned char*>(iq), 0, hop, avg, window, gain, power, rows, jobs_dev, njobs, s);
}

}  // namespace mdc

using namespace mdc;

int64_t mdc_iq_spectrogram_rows(int64_t pairs_in, int nfft, int64_t hop, int avg) {
    const int rc = spec_shape_check("mdc_iq_spectrogram_rows", pairs_in, nfft, hop, avg);
    return rc != MDC_OK ? (int64_t)rc : spec_rows(pairs_in, nfft, hop, avg);
}

// both entry points: order 1 is mdc_iq_spectrogram
static int spec_run(const char* who, const void* iq_dev, int format, int64_t pairs_in, int order, int nfft, int64_t hop, int avg, const int16_t* window_dev,
                    float scale, float* power_dev, int64_t rows, void* hip_stream) {
    int rc = iq_format_known(who, format);
    if (rc != MDC_OK) return rc;
    if (order != 0 && order != 1 && order != 2 && order != 4) { set_error("%s: order must be 0 (envelope), 1, 2 or 4 (got %d)", who, order); return MDC_EINVAL; }
    if ((rc = spec_shape_check(who, pairs_in, nfft, hop, avg)) != MDC_OK) return rc;
    if (!(scale > 0.f) || !(scale <= 3.402823466e38f)) { set_error("%s: scale must be finite and > 0 (got %g)", who, (double)scale); return MDC_EINVAL; }
    if (rows != spec_rows(pairs_in, nfft, hop, avg)) {
        set_error("%s: rows is %lld, mdc_iq_spectrogram_rows gives %lld", who, (long long)rows, (long long)spec_rows(pairs_in, nfft, hop, avg));
        return MDC_EINVAL;
    }
    if ((rc = iq_pair_aligned(who, "iq_dev", format, iq_dev)) != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "window_dev", window_dev, 2)) != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "power_dev", power_dev, 4)) != MDC_OK) return rc;
    if (rows == 0) return MDC_OK;
    if (!iq_dev || !window_dev || !power_dev) { set_error("%s: null buffer", who); return MDC_EINVAL; }
    const float gain = (float)((double)scale / (double)avg);
    const int log2n = pow2_log2(nfft, kSpecMinLog2, kSpecMaxLog2);
    const unsigned char* p = static_cast<const unsigned char*>(iq_dev);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return guarded(who, [&]() -> int { return spec_dispatch(format, order, log2n, p, pairs_in, hop, avg, window_dev, gain, power_dev, rows, nullptr, 0, s); });
}

int mdc_iq_spectrogram(const void* iq_dev, int format, int64_t pairs_in, int nfft, int64_t hop, int avg, const int16_t* window_dev, float scale,
                       float* power_dev, int64_t rows, void* hip_stream) {
    return spec_run("mdc_iq_spectrogram", iq_dev, format, pairs_in, 1, nfft, hop, avg, window_dev, scale, power_dev, rows, hip_stream);
}

int mdc_iq_line_spectrum(const void* iq_dev, int format, int64_t pairs_in, int order, int nfft, int64_t hop, int avg, const int16_t* window_dev, float scale,
                         float* power_dev, int64_t rows, void* hip_stream) {
    return spec_run("mdc_iq_line_spectrum", iq_dev, format, pairs_in, order, nfft, hop, avg, window_dev, scale, power_dev, rows, hip_stream);
}
