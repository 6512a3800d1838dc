// The power-of-two transform of the device front-end, over a complex f32 image in LDS: the spectrogram (iq_spectrogram.hip: one
// transform per work-group, up to two butterflies per thread) and the channelizer (iq_channelizer.hip: 1024 / M transforms side by
// side, one butterfly per thread) call the code below; the float32 numpy restatement is tests/iq_fft_f32_ref.py.
//
//   passes    Stockham autosort, decimation in frequency, radix 4: butterfly t of a pass with stride s = 4^pass reads elements
//             t + k n/4 (k = 0..3: contiguous over the lanes), multiplies outputs 1..3 by w^(j), w^(2j), w^(3j), j = t with its
//             low log2(s) bits cleared, w = e^{-2 pi i / n}, and writes elements q + 4 (t - q) + k s, q = t mod s.  In place:
//             every thread reads all its butterflies, barrier, writes them, barrier (fft_stored_passes).  An odd log2(n) ends with
//             one radix-2 pass.  The LAST pass writes nothing (fft_last_pass): its outputs are bins t + k n/4 (radix 4; t + k n/2
//             for radix 2) in natural order, and the caller takes them from registers.
//   twiddles  three tables w^j, w^2j, w^3j (j < n/4) in LDS, filled once per work-group (fft_fill_twiddles) from the first
//             quadrant of the 4096-point circle (iq_fft_twiddles.h: float64 cos / sin rounded to f32 by tools/gen_fft_twiddles.py;
//             the other quadrants are swaps and sign changes, exact).  Nothing is computed with device sines.
//   image     one element of padding after every 16 (fft_slot): the writes of the first pass, element stride 4 over the lanes,
//             would otherwise put each 16-lane group of a 64-bit store on 4 of its 16 bank pairs.  A transform's elements start
//             at any element `eb` of the image: the padding goes by the element's index in the image, not in the transform.
// What differs between the callers is an argument: where a transform starts, which butterflies a thread owns, and what becomes of
// the last pass's outputs.  A thread owns the butterflies t0 + i STRIDE, i < B, of those below the pass's count.
// Everything here has internal linkage: each translation unit that includes it carries its own copy of the table.
#pragma once
#include "mdc_internal.h"

namespace mdc {

namespace {

constexpr int kFftCircleLog2 = 12;                           // the table's circle: the largest transform
constexpr int kFftQuadrant = 1 << (kFftCircleLog2 - 2);      // entries of iq_fft_twiddles.h

__device__ const unsigned d_fft_tw[2 * kFftQuadrant] = {
#include "iq_fft_twiddles.h"
};

__host__ __device__ constexpr int fft_slot(int e) { return e + (e >> 4); }
__host__ __device__ constexpr int fft_stored_pass_count(int log2n) { return (log2n & 1) != 0 ? log2n / 2 : log2n / 2 - 1; }
__host__ __device__ constexpr int fft_last_radix(int log2n) { return (log2n & 1) != 0 ? 2 : 4; }

// e^{-2 pi i J / 4096}, 0 <= J < 3072
__device__ __forceinline__ float2 fft_twiddle(int J) {
    const int j = J & (kFftQuadrant - 1), quadrant = J >> (kFftCircleLog2 - 2);
    const float c = __uint_as_float(d_fft_tw[2 * j]), s = __uint_as_float(d_fft_tw[2 * j + 1]);
    return quadrant == 0 ? make_float2(c, -s) : quadrant == 1 ? make_float2(-s, -c) : make_float2(-c, s);
}

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }
__device__ __forceinline__ float2 cmuli(float2 a) { return make_float2(-a.y, a.x); }      // a * i

// the three tables of a 2^LOG2N-point transform into tw[3 n/4], by T threads (no barrier)
template <int LOG2N, int T>
__device__ __forceinline__ void fft_fill_twiddles(float2* tw, int tid) {
    constexpr int NB = (1 << LOG2N) / 4;
    for (int j = tid; j < NB; j += T) {
        const int J = j << (kFftCircleLog2 - LOG2N);
        tw[j] = fft_twiddle(J);
        tw[NB + j] = fft_twiddle(2 * J);
        tw[2 * NB + j] = fft_twiddle(3 * J);
    }
}

// the radix-4 butterfly on elements e + k n/4 of the image, before the twiddles: out(k, value) for k = 0..3, in that order
template <int LOG2N, class Out>
__device__ __forceinline__ void fft_butterfly4(const float2* x, int e, Out out) {
    constexpr int NB = (1 << LOG2N) / 4;
    const float2 a = x[fft_slot(e)], b = x[fft_slot(e + NB)], c = x[fft_slot(e + 2 * NB)], d = x[fft_slot(e + 3 * NB)];
    const float2 apc = cadd(a, c), amc = csub(a, c), bpd = cadd(b, d), jbmd = cmuli(csub(b, d));
    out(0, cadd(apc, bpd));
    out(1, csub(amc, jbmd));
    out(2, csub(apc, bpd));
    out(3, cadd(amc, jbmd));
}

// every pass but the last of the transform on elements eb .. eb + n - 1.  The caller's barrier stands between the image's last
// write and this; on return the image is ready for fft_last_pass.  y holds a pass's outputs across its barrier.  It is the
// caller's, declared inside its loop over segments or groups, because where it lives decides bits: as a local of this function
// hipcc promotes it to registers before the function is inlined, and the spectrogram's 64- and 128-point kernels, whose
// butterflies are guarded, then contract a different set of multiply-adds (read in the ISA) than the results on record.
template <int LOG2N, int B, int STRIDE>
__device__ __forceinline__ void fft_stored_passes(float2* x, const float2* tw, int eb, int t0, float2 (&y)[B][4]) {
    constexpr int NB = (1 << LOG2N) / 4;
    constexpr bool kWhole = B * STRIDE == NB;      // else the pass has fewer butterflies than the threads own
#pragma unroll
    for (int pass = 0; pass < fft_stored_pass_count(LOG2N); ++pass) {
        const int s = 1 << (2 * pass);
#pragma unroll
        for (int i = 0; i < B; ++i) {
            const int t = t0 + i * STRIDE;
            if (kWhole || t < NB) {
                const int j = t & ~(s - 1);
                fft_butterfly4<LOG2N>(x, eb + t, [&](int k, float2 v) { y[i][k] = k == 0 ? v : cmul(v, tw[(k - 1) * NB + j]); });
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < B; ++i) {
            const int t = t0 + i * STRIDE;
            if (kWhole || t < NB) {
                const int q = t & (s - 1), base = eb + q + 4 * (t - q);
#pragma unroll
                for (int k = 0; k < 4; ++k) x[fft_slot(base + k * s)] = y[i][k];
            }
        }
        __syncthreads();
    }
}

// the last pass, R = fft_last_radix(LOG2N): stride n/R, no twiddles, n/R butterflies.  Output k of the thread's i-th butterfly t is
// bin t + k n/R of the transform: emit(i, k, bin, value), in that order of k and i.
template <int LOG2N, int B, int STRIDE, class Emit>
__device__ __forceinline__ void fft_last_pass(const float2* x, int eb, int t0, Emit emit) {
    constexpr int R = fft_last_radix(LOG2N), NL = (1 << LOG2N) / R;
    constexpr bool kWhole = B * STRIDE == NL;
#pragma unroll
    for (int i = 0; i < B; ++i) {
        const int t = t0 + i * STRIDE;
        if (kWhole || t < NL) {
            if constexpr (R == 4) {
                fft_butterfly4<LOG2N>(x, eb + t, [&](int k, float2 v) { emit(i, k, t + k * NL, v); });
            } else {
                const float2 a = x[fft_slot(eb + t)], b = x[fft_slot(eb + t + NL)];
                emit(i, 0, t, cadd(a, b));
                emit(i, 1, t + NL, csub(a, b));
            }
        }
    }
}

}  // namespace

}  // namespace mdc
