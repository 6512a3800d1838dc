// mdc_iq_channelizer -- a polyphase filter bank: all M evenly spaced channels of an integer I/Q capture in one pass (include/mdc.h,
// "channelizer"; the float64 numpy restatement is tests/iq_channelizer_ref.py).  Per output step j the prototype filter runs ONCE
// -- T integer multiply-adds folded into M branch sums -- and one M-point transform turns the branch sums into the M channels.
//
//   tile      a work-group of 256 threads owns kJ = max(16, 1024 / M) consecutive output steps (chan_tile_steps) and walks them in
//             groups of G = 1024 / M steps: a group is 1024 complex elements, whatever M is, so every thread has work at every M
//             (M = 16: 64 transforms side by side).  Work-groups stride over the tiles (grid cap kChanGridCap).
//   sums      thread (g, q) of a group, q < M / 4, owns the taps t = 4 q + e + i M (e < 4, i = 0, 1, ...) of step j: per i one
//             quad load of the capture (iq_mix.h's load_quad: one unaligned 8- or 16-byte vector load, widened to 16-bit full
//             scale) and one 8-byte load of four taps, eight 24-bit multiply-adds (exact: every factor is below 2^16).  Whole
//             quads of taps need no bound on the capture (j D + T <= P) and run four deep; the filter's last, partial quad
//             goes tap by tap, bounded.  The lanes of a step read the capture and the taps contiguously.  Its four sums belong
//             to the residues (4 q + e + first_index + j D) mod M: the rotation is in the LDS address the sums are written to,
//             as f32.  Neither the capture nor the taps are staged in LDS: a tile's (kJ - 1) D + T pairs are read T / D times
//             each by the same work-group and come from L1 / L2 after the first.  Taps past T are zero, pairs
//             past the capture are never read: memory-safe for any taps; sums that break the header's per-residue
//             precondition wrap (the accumulation is unsigned).
//   passes    iq_fft.h's transform, G of them side by side in one image: transform g starts at element g M, and butterfly b of a
//             pass is transform b / (M / 4), index b mod (M / 4).  With 256 threads and 1024 elements a radix-4 pass is one
//             butterfly per thread, the radix-2 pass that ends an odd log2 M two.
//   output    the last pass keeps its outputs in registers: out = clamp(rint(Y 2^-(15+s))) as an int16 pair, written to an LDS
//             image [channel][step of the tile] (chan_image_slot: columns swizzled against bank conflicts).  When the tile is
//             done the image leaves channel by channel: runs of kJ pairs (>= 64 bytes) per channel row, one dword per lane.
//   LDS       1088 complex f32 (8.5 KiB) + 3 M / 4 twiddles + M kJ dwords: 13 KiB at M = 16, 78.5 KiB at M = 1024 (two
//             work-groups per CU).
// Every step's arithmetic is the same whatever tile, group or slot it lands in -- integer sums are exact and the transform of a
// slot touches that slot's elements only --: the same bits on every run, for every split of a capture.
// The call only enqueues; vector memory for every store.
#include "iq_fft.h"
#include "iq_mix.h"

namespace mdc {

namespace {

constexpr int kChanMinLog2 = 3, kChanMaxLog2 = 10, kChanTapsPerChannel = 16, kChanMaxShift = 15;
constexpr long kChanGridCap = 2048;      // work-groups; beyond it the kernel strides (_cabi.CHANNELIZER_GRID_CAP)
constexpr int kChanThreads = 256;
constexpr int kChanGroupElems = 1024;    // complex elements of one group of transforms: 4 per thread

__host__ __device__ constexpr int chan_tile_steps(int log2m) { return kChanGroupElems >> log2m < 16 ? 16 : kChanGroupElems >> log2m; }

// the tile's output image: channel c's row of J dwords, its columns XORed with the channel's bits above SWZ.  Unswizzled rows put
// the last pass's writes (a wave: consecutive channels of one column, row stride 16 dwords at M >= 64) on 4 of the 64 banks; with
// SWZ = log2(64 / J) (0 from J = 64 on) 64 consecutive channels of a column, and 64 / J whole rows, each cover all 64.  No padding:
// at M = 1024 two work-groups share a CU's LDS only without it.
template <int J, int SWZ> __device__ __forceinline__ int chan_image_slot(int c, int jj) { return c * J + (jj ^ ((c >> SWZ) & (J - 1))); }

// clamp(rint(y * scale)) of both components as one int16 pair
__device__ __forceinline__ unsigned chan_pack(float2 y, float scale) {
    const float r = fminf(fmaxf(rintf(y.x * scale), -32768.f), 32767.f), i = fminf(fmaxf(rintf(y.y * scale), -32768.f), 32767.f);
    return ((unsigned)(int)r & 0xFFFFu) | ((unsigned)(int)i << 16);
}

template <int FMT, int LOG2M>
__global__ __launch_bounds__(kChanThreads) void iq_channelizer_kernel(const unsigned char* __restrict__ iq, long pairs, unsigned rot0, int decimate,
                                                                     const short* __restrict__ taps, int ntaps, float scale,
                                                                     unsigned* __restrict__ out, long n_out) {
    constexpr int M = 1 << LOG2M, NB = M / 4, G = kChanGroupElems / M, kJ = chan_tile_steps(LOG2M);
    constexpr int kSwz = kJ >= 64 ? 0 : kJ == 32 ? 1 : 2;      // chan_image_slot
    constexpr unsigned NL = M / fft_last_radix(LOG2M);         // butterflies of a transform's last pass: one per thread, or two
    static_assert(kJ % G == 0 && G * NB == kChanThreads, "a group is one radix-4 butterfly per thread");
    __shared__ float2 x[fft_slot(kChanGroupElems)];
    __shared__ float2 tw[3 * NB];
    __shared__ unsigned res[M * kJ];
    const int tid = threadIdx.x;
    const int g = tid >> (LOG2M - 2), q = tid & (NB - 1);      // this thread's transform of the group, and its quad / butterfly in it
    fft_fill_twiddles<LOG2M, kChanThreads>(tw, tid);
    const long tiles = (n_out + kJ - 1) / kJ;
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long j0 = tile * kJ;
        for (int grp = 0; grp < kJ / G; ++grp) {
            const long j = j0 + grp * G + g;
            unsigned ar[4] = {0u, 0u, 0u, 0u}, ai[4] = {0u, 0u, 0u, 0u};
            if (j < n_out) {
                const long in0 = j * decimate;
                // whole quads of taps: j D + T <= P for every step, so their pairs lie inside the capture and load_quad needs no
                // bound (its partial-quad branch folds away; the loads of several iterations are in flight together)
                int t = 4 * q;
#pragma unroll 4
                for (; t + 4 <= ntaps; t += M) {
                    int I[4], Q[4];
                    load_quad<FMT>(iq, in0 + t, 0x7FFFFFFFFFFFFFFFL, I, Q);
                    short h[4];
                    __builtin_memcpy(h, taps + t, sizeof(h));
#pragma unroll
                    for (int e = 0; e < 4; ++e) {      // |I|, |Q|, |h| <= 2^15: the 24-bit multiply is exact
                        ar[e] += (unsigned)__mul24(I[e], (int)h[e]);
                        ai[e] += (unsigned)__mul24(Q[e], (int)h[e]);
                    }
                }
                if (t < ntaps) {      // the filter's last, partial quad: tap by tap, pairs past the capture read nothing
                    int I[4], Q[4];
                    load_quad<FMT>(iq, in0 + t, pairs, I, Q);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int h = t + e < ntaps ? (int)taps[t + e] : 0;
                        ar[e] += (unsigned)__mul24(I[e], h);
                        ai[e] += (unsigned)__mul24(Q[e], h);
                    }
                }
            }
            const int rot = (int)((rot0 + (unsigned)((unsigned long)j * (unsigned long)decimate)) & (unsigned)(M - 1));
            __syncthreads();      // the twiddles are in place; the previous group's last pass has read its image
#pragma unroll
            for (int e = 0; e < 4; ++e)
                x[fft_slot(g * M + ((4 * q + e + rot) & (M - 1)))] = make_float2((float)(int)ar[e], (float)(int)ai[e]);
            __syncthreads();
            float2 y[1][4];
            fft_stored_passes<LOG2M, 1, NB>(x, tw, g * M, q, y);
            // the last pass: butterfly b of the group is transform b / NL, index b mod NL (radix 4: g and q again); its outputs are
            // the channels of the step in column grp G + b / NL of the tile's image
#pragma unroll
            for (int i = 0; i < G * (int)NL / kChanThreads; ++i) {
                const unsigned b = tid + i * kChanThreads;
                const int gl = (int)(b / NL), jj = grp * G + gl;
                fft_last_pass<LOG2M, 1, (int)NL>(x, gl * M, (int)(b % NL), [&](int, int, int channel, float2 v) {
                    res[chan_image_slot<kJ, kSwz>(channel, jj)] = chan_pack(v, scale);
                });
            }
        }
        __syncthreads();      // the tile's image is complete
        const long left = n_out - j0;
        const int valid = left < kJ ? (int)left : kJ;
        for (int idx = tid; idx < M * kJ; idx += kChanThreads) {
            const int k = idx / kJ, jj = idx % kJ;
            if (jj < valid) out[(long)k * n_out + j0 + jj] = res[chan_image_slot<kJ, kSwz>(k, jj)];
        }
        // (the next tile writes the image only in its last passes, behind several barriers)
    }
}

template <int FMT, int LOG2M>
int chan_launch(const unsigned char* iq, int64_t pairs, unsigned rot0, int decimate, const int16_t* taps, int ntaps, float scale, int16_t* out,
                int64_t n_out, hipStream_t s) {
    const long tiles = (n_out + chan_tile_steps(LOG2M) - 1) / chan_tile_steps(LOG2M);
    const dim3 g((unsigned)(tiles < kChanGridCap ? tiles : kChanGridCap)), b(kChanThreads);
    hipLaunchKernelGGL((iq_channelizer_kernel<FMT, LOG2M>), g, b, 0, s, iq, (long)pairs, rot0, decimate, reinterpret_cast<const short*>(taps), ntaps, scale,
                       reinterpret_cast<unsigned*>(out), (long)n_out);
    MDC_HIP(hipGetLastError());
    return MDC_OK;
}

int chan_shape_check(const char* who, int64_t pairs, int channels, int ntaps, int decimate) {
    if (pow2_log2(channels, kChanMinLog2, kChanMaxLog2) < 0) {
        set_error("%s: channels must be a power of two in %d..%d (got %d)", who, 1 << kChanMinLog2, 1 << kChanMaxLog2, channels);
        return MDC_EINVAL;
    }
    if (decimate < 1 || decimate > channels) { set_error("%s: decimate must be in 1..channels = %d (got %d)", who, channels, decimate); return MDC_EINVAL; }
    if (ntaps < 1 || ntaps > kChanTapsPerChannel * channels) {
        set_error("%s: ntaps must be in 1..%d (16 per channel; got %d)", who, kChanTapsPerChannel * channels, ntaps);
        return MDC_EINVAL;
    }
    if (pairs < 0) { set_error("%s: negative pair count", who); return MDC_EINVAL; }
    return MDC_OK;
}

}  // namespace

}  // namespace mdc

using namespace mdc;

int64_t mdc_iq_channelizer_out_count(int64_t pairs_in, int channels, int ntaps, int decimate) {
    const int rc = chan_shape_check("mdc_iq_channelizer_out_count", pairs_in, channels, ntaps, decimate);
    return rc != MDC_OK ? (int64_t)rc : iq_span_count(pairs_in, ntaps, decimate);
}

int mdc_iq_channelizer(const void* iq_dev, int format, int64_t pairs_in, int64_t first_index, int channels, int decimate, const int16_t* taps_dev,
                       int ntaps, int tap_shift, int16_t* out_dev, int64_t n_out, void* hip_stream) {
    int rc = iq_format_known("mdc_iq_channelizer", format);
    if (rc != MDC_OK) return rc;
    if ((rc = chan_shape_check("mdc_iq_channelizer", pairs_in, channels, ntaps, decimate)) != MDC_OK) return rc;
    if (tap_shift < 0 || tap_shift > kChanMaxShift) { set_error("mdc_iq_channelizer: tap_shift must be in 0..%d (got %d)", kChanMaxShift, tap_shift); return MDC_EINVAL; }
    if (first_index < 0) { set_error("mdc_iq_channelizer: negative first_index"); return MDC_EINVAL; }
    if (n_out != iq_span_count(pairs_in, ntaps, decimate)) {
        set_error("mdc_iq_channelizer: n_out is %lld, mdc_iq_channelizer_out_count gives %lld", (long long)n_out,
                  (long long)iq_span_count(pairs_in, ntaps, decimate));
        return MDC_EINVAL;
    }
    if ((rc = iq_pair_aligned("mdc_iq_channelizer", "iq_dev", format, iq_dev)) != MDC_OK) return rc;
    if ((rc = iq_aligned("mdc_iq_channelizer", "taps_dev", taps_dev, 2)) != MDC_OK) return rc;
    if ((rc = iq_aligned("mdc_iq_channelizer", "out_dev", out_dev, 4)) != MDC_OK) return rc;
    if (n_out == 0) return MDC_OK;
    if (!iq_dev || !taps_dev || !out_dev) { set_error("mdc_iq_channelizer: null buffer"); return MDC_EINVAL; }
    const int log2m = pow2_log2(channels, kChanMinLog2, kChanMaxLog2);
    const unsigned rot0 = (unsigned)(first_index & (int64_t)(channels - 1));
    float scale = 1.f;
    for (int i = 0; i < 15 + tap_shift; ++i) scale *= 0.5f;      // 2^-(15+s), exact
    const unsigned char* p = static_cast<const unsigned char*>(iq_dev);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return guarded("mdc_iq_channelizer", [&]() -> int {
        return with_format(format, [&](auto fmt) {
            return with_log2<kChanMinLog2, kChanMaxLog2>(log2m, [&](auto l2) {
                return chan_launch<decltype(fmt)::value, decltype(l2)::value>(p, pairs_in, rot0, decimate, taps_dev, ntaps, scale, out_dev, n_out, s);
            });
        });
    });
}
