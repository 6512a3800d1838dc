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
//   passes    Stockham autosort, decimation in frequency, radix 4: butterfly t of a pass with stride s = 4^pass reads elements
//             t + k nfft/4 (k = 0..3: contiguous over the lanes), multiplies outputs 1..3 by w^(j), w^(2j), w^(3j), j = t with its
//             low log2(s) bits cleared, w = e^{-2 pi i / nfft}, and writes elements q + 4 (t - q) + k s, q = t mod s.  In place:
//             every thread reads all its butterflies, barrier, writes them, barrier.  An odd log2(nfft) ends with one radix-2 pass.
//             The LAST pass writes nothing: its outputs are bins t + k nfft/4 (radix 4; t + k nfft/2 for radix 2) in natural order,
//             and the thread adds their squared magnitudes to its accumulators.  The row's store is then coalesced.
//   twiddles  three tables w^j, w^2j, w^3j (j < nfft/4) in LDS, filled once per work-group from the first quadrant of the
//             4096-point circle (iq_fft_twiddles.h: float64 cos / sin rounded to f32 by tools/gen_fft_twiddles.py; the other
//             quadrants are swaps and sign changes, exact).  Nothing is computed with device sines.
//   LDS       complex f32 elements, one element of padding after every 16 (spec_slot): the writes of the first pass, element
//             stride 4 over the lanes, would otherwise put each 16-lane group of a 64-bit store on 4 of its 16 bank pairs.  nfft = 4096:
//             34 KiB of image + 24 KiB of twiddles, two work-groups per CU.
// mdc_iq_line_spectrum is the same kernel with ORDER != 1: the staging alone differs (spec_stage; include/mdc.h, "line spectrum";
// tests/iq_line_ref.py), everything from the image on is shared -- DESIGN.md 5.19.
// mdc_iq_line_spectra (iq_line_spectra.hip) is the same kernel again, handed a JOB TABLE: its rows are then the jobs' rows back to
// back, and a work-group looks its row's job up (a binary search of the table's first_row column, uniform over the work-group)
// and runs the row on the job's slice -- base pointer iq + first_pair, bound `pairs`, the row counted from the job's first.  The
// very instructions that serve a call on the slice compute the row, so its bits are that call's by construction, and no pair
// outside the job is read: every segment of a row the rows function counts lies inside the bound.
// The call only enqueues; vector memory for every store.
#include "iq_mix.h"

namespace mdc {

namespace {

constexpr int kSpecMinLog2 = 6, kSpecMaxLog2 = 12, kSpecMaxAvg = 4096;
constexpr long kSpecGridCap = 2048;      // work-groups; beyond it the kernel strides (_cabi.SPECTROGRAM_GRID_CAP)
constexpr int kTwQuadrant = 1024;        // entries of iq_fft_twiddles.h: a quarter of the 4096-point circle

__device__ const unsigned d_tw[2 * kTwQuadrant] = {
#include "iq_fft_twiddles.h"
};

__host__ __device__ constexpr int spec_threads(int log2n) { return (1 << log2n) / 4 < 64 ? 64 : (1 << log2n) / 4 > 512 ? 512 : (1 << log2n) / 4; }
__host__ __device__ constexpr int spec_slot(int e) { return e + (e >> 4); }

// e^{-2 pi i J / 4096}, 0 <= J < 3072
__device__ __forceinline__ float2 spec_twiddle(int J) {
    const int j = J & (kTwQuadrant - 1), quadrant = J >> 10;
    const float c = __uint_as_float(d_tw[2 * j]), s = __uint_as_float(d_tw[2 * j + 1]);
    return quadrant == 0 ? make_float2(c, -s) : quadrant == 1 ? make_float2(-s, -c) : make_float2(-c, s);
}

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }
__device__ __forceinline__ float2 cmuli(float2 a) { return make_float2(-a.y, a.x); }      // a * i
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
    constexpr bool kOdd = (LOG2N & 1) != 0;
    constexpr int kStoredPasses = kOdd ? LOG2N / 2 : LOG2N / 2 - 1;
    constexpr int B2 = N / 2 / T;                    // radix-2 butterflies per thread in the last pass of an odd log2
    __shared__ float2 x[spec_slot(N)];
    __shared__ float2 tw[3 * NB];
    const int tid = threadIdx.x;
    for (int j = tid; j < NB; j += T) {
        const int J = j << (kSpecMaxLog2 - LOG2N);
        tw[j] = spec_twiddle(J);
        tw[NB + j] = spec_twiddle(2 * J);
        tw[2 * NB + j] = spec_twiddle(3 * J);
    }

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
        float acc[4 * B];
#pragma unroll
        for (int i = 0; i < 4 * B; ++i) acc[i] = 0.f;
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
                    for (int e = 0; e < 4; ++e) x[spec_slot(4 * q + e)] = spec_stage<ORDER>(I[e], Q[e], (int)w[e]);
                }
            }
            __syncthreads();
#pragma unroll
            for (int pass = 0; pass < kStoredPasses; ++pass) {
                const int s = 1 << (2 * pass);
                float2 y[B][4];
#pragma unroll
                for (int i = 0; i < B; ++i) {
                    const int t = tid + i * T;
                    if (kWhole || t < NB) {
                        const float2 a = x[spec_slot(t)], b = x[spec_slot(t + NB)], c = x[spec_slot(t + 2 * NB)], d = x[spec_slot(t + 3 * NB)];
                        const float2 apc = cadd(a, c), amc = csub(a, c), bpd = cadd(b, d), jbmd = cmuli(csub(b, d));
                        const int j = t & ~(s - 1);
                        y[i][0] = cadd(apc, bpd);
                        y[i][1] = cmul(csub(amc, jbmd), tw[j]);
                        y[i][2] = cmul(csub(apc, bpd), tw[NB + j]);
                        y[i][3] = cmul(cadd(amc, jbmd), tw[2 * NB + j]);
                    }
                }
                __syncthreads();
#pragma unroll
                for (int i = 0; i < B; ++i) {
                    const int t = tid + i * T;
                    if (kWhole || t < NB) {
                        const int q = t & (s - 1), base = q + 4 * (t - q);
#pragma unroll
                        for (int k = 0; k < 4; ++k) x[spec_slot(base + k * s)] = y[i][k];
                    }
                }
                __syncthreads();
            }
            if (!kOdd) {      // the last radix-4 pass: stride nfft/4, no twiddles, bins t + k nfft/4
#pragma unroll
                for (int i = 0; i < B; ++i) {
                    const int t = tid + i * T;
                    if (kWhole || t < NB) {
                        const float2 a = x[spec_slot(t)], b = x[spec_slot(t + NB)], c = x[spec_slot(t + 2 * NB)], d = x[spec_slot(t + 3 * NB)];
                        const float2 apc = cadd(a, c), amc = csub(a, c), bpd = cadd(b, d), jbmd = cmuli(csub(b, d));
                        acc[4 * i + 0] += norm2(cadd(apc, bpd));
                        acc[4 * i + 1] += norm2(csub(amc, jbmd));
                        acc[4 * i + 2] += norm2(csub(apc, bpd));
                        acc[4 * i + 3] += norm2(cadd(amc, jbmd));
                    }
                }
            } else {          // the last radix-2 pass: stride nfft/2, bins t and t + nfft/2
#pragma unroll
                for (int i = 0; i < B2; ++i) {
                    const int t = tid + i * T;
                    const float2 a = x[spec_slot(t)], b = x[spec_slot(t + N / 2)];
                    acc[2 * i + 0] += norm2(cadd(a, b));
                    acc[2 * i + 1] += norm2(csub(a, b));
                }
            }
        }
        float* out = power + grow * N;
        if (!kOdd) {
#pragma unroll
            for (int i = 0; i < B; ++i) {
                const int t = tid + i * T;
                if (kWhole || t < NB) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) out[t + k * NB] = acc[4 * i + k] * gain;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < B2; ++i) {
                const int t = tid + i * T;
                out[t] = acc[2 * i] * gain;
                out[t + N / 2] = acc[2 * i + 1] * gain;
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

template <int FMT, int ORDER>
int spec_launch_fmt(int log2n, const unsigned char* iq, int64_t pairs, int64_t hop, int avg, const int16_t* window, float gain, float* power, int64_t rows,
                    const mdc_iq_line_job* jobs, int64_t njobs, hipStream_t s) {
    switch (log2n) {
        case 6: return spec_launch<FMT, 6, ORDER>(iq, pairs, hop, avg, window, gain, power, rows, jobs, njobs, s);
        case 7: return spec_launch<FMT, 7, ORDER>(iq, pairs, hop, avg, window, gain, power, rows, jobs, njobs, s);
        case 8: return spec_launch<FMT, 8, ORDER>(iq, pairs, hop, avg, window, gain, power, rows, jobs, njobs, s);
        case 9: return spec_launch<FMT, 9, ORDER>(iq, pairs, hop, avg, window, gain, power, rows, jobs, njobs, s);
        case 10: return spec_launch<FMT, 10, ORDER>(iq, pairs, hop, avg, window, gain, power, rows, jobs, njobs, s);
        case 11: return spec_launch<FMT, 11, ORDER>(iq, pairs, hop, avg, window, gain, power, rows, jobs, njobs, s);
        default: return spec_launch<FMT, 12, ORDER>(iq, pairs, hop, avg, window, gain, power, rows, jobs, njobs, s);
    }
}

int spec_log2(int nfft) {      // log2 of a power of two in 64..4096, else -1
    for (int l = kSpecMinLog2; l <= kSpecMaxLog2; ++l)
        if (nfft == 1 << l) return l;
    return -1;
}

int spec_shape_check(const char* who, int64_t pairs, int nfft, int64_t hop, int avg) {
    if (spec_log2(nfft) < 0) { set_error("%s: nfft must be a power of two in %d..%d (got %d)", who, 1 << kSpecMinLog2, 1 << kSpecMaxLog2, nfft); return MDC_EINVAL; }
    if (hop < 1) { set_error("%s: hop must be >= 1 pair (got %lld)", who, (long long)hop); return MDC_EINVAL; }
    if (avg < 1 || avg > kSpecMaxAvg) { set_error("%s: avg must be in 1..%d (got %d)", who, kSpecMaxAvg, avg); return MDC_EINVAL; }
    if (pairs < 0) { set_error("%s: negative pair count", who); return MDC_EINVAL; }
    return MDC_OK;
}

int64_t spec_rows(int64_t pairs, int nfft, int64_t hop, int avg) {
    const int64_t segs = pairs >= nfft ? (pairs - nfft) / hop + 1 : 0;
    return segs / avg;
}

// format and order as template arguments; jobs == nullptr: the rows of the capture itself
int spec_dispatch(int format, int order, int log2n, const unsigned char* p, int64_t pairs, int64_t hop, int avg, const int16_t* window, float gain, float* power,
                  int64_t rows, const mdc_iq_line_job* jobs, int64_t njobs, hipStream_t s) {
    return with_format(format, [&](auto fmt) {
        constexpr int F = decltype(fmt)::value;
        switch (order) {
            case 0: return spec_launch_fmt<F, 0>(log2n, p, pairs, hop, avg, window, gain, power, rows, jobs, njobs, s);
            case 1: return spec_launch_fmt<F, 1>(log2n, p, pairs, hop, avg, window, gain, power, rows, jobs, njobs, s);
            case 2: return spec_launch_fmt<F, 2>(log2n, p, pairs, hop, avg, window, gain, power, rows, jobs, njobs, s);
            default: return spec_launch_fmt<F, 4>(log2n, p, pairs, hop, avg, window, gain, power, rows, jobs, njobs, s);
        }
    });
}

}  // namespace

// what iq_line_spectra.hip needs of this file (mdc_internal.h)
int iq_spec_shape_check(const char* who, int64_t pairs, int nfft, int64_t hop, int avg) { return spec_shape_check(who, pairs, nfft, hop, avg); }
int64_t iq_spec_rows(int64_t pairs, int nfft, int64_t hop, int avg) { return spec_rows(pairs, nfft, hop, avg); }
int iq_spec_jobs_launch(const void* iq, int format, int order, int nfft, int64_t hop, int avg, const int16_t* window, float gain, float* power, int64_t rows,
                        const mdc_iq_line_job* jobs_dev, int64_t njobs, hipStream_t s) {
    return spec_dispatch(format, order, spec_log2(nfft), static_cast<const unsigned char*>(iq), 0, hop, avg, window, gain, power, rows, jobs_dev, njobs, s);
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
    if ((reinterpret_cast<uintptr_t>(window_dev) & 1) != 0) { set_error("%s: window_dev must be 2-byte aligned", who); return MDC_EINVAL; }
    if ((reinterpret_cast<uintptr_t>(power_dev) & 3) != 0) { set_error("%s: power_dev must be 4-byte aligned", who); return MDC_EINVAL; }
    if (rows == 0) return MDC_OK;
    if (!iq_dev || !window_dev || !power_dev) { set_error("%s: null buffer", who); return MDC_EINVAL; }
    const float gain = (float)((double)scale / (double)avg);
    const int log2n = spec_log2(nfft);
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
