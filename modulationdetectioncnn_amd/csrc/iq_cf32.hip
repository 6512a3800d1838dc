// mdc_iq_cf32_histogram / mdc_iq_cf32_quantize -- a complex float32 capture at the door: the exact statistics of its magnitudes (a
// 256-bin histogram of every component's biased exponent byte) and a one-rounding quantiser into an ordinary MDC_IQ_CI16 stream
// (include/mdc.h, "float captures"; the numpy restatement is tests/iq_cf32_ref.py).  Two pointwise streams over the capture; a
// work-group of 256 lanes takes kCfGroupPairs = 1024 pairs per stride step, four per lane, at most kCfGridCap work-groups:
//
//   histogram  iq_cf32_histogram_kernel.  The capture is aligned to a pair (8 bytes) only: the pair in front of the first 16-byte
//              boundary (the head, 0 or 1) and the pair behind the last whole 16-byte group (the tail, 0 or 1) go to one lane each of
//              work-group 0 as 8-byte loads; between them every lane takes two aligned 16-byte loads a step, 4 KiB apart, so each
//              wave instruction reads 1 KiB contiguous.  Counting is per work-group in LDS: a real signal puts nearly all components
//              into three to six adjacent bins, and 64 lanes of a wave adding to ONE LDS word serialise, so the work-group keeps
//              kCfReplicas = 16 histograms, lane L adding into replica L % 16, laid out bin-major (word = bin * 16 + replica):
//              equal bins of a wave spread over 16 words (at most 4 lanes each), and four adjacent bins cover all 64 banks.
//              At the end lane b sums bin b's replicas (rotated by b, so the 64 lanes of a wave read 64 banks) and adds a nonzero
//              sum to hist[b] with one 64-bit global atomic; empty bins add nothing.  Counts are integers: any order, same bits.
//              A replica word is a uint32 and counts at most the components the work-group sees:
//                  2 * kCfGroupPairs * ceil(ceil(pairs / kCfGroupPairs) / kCfGridCap) + 4 <= 2^11 * 2^20 + 4 < 2^32
//              for pairs <= kCfMaxPairs = 2^40 (8 TiB of capture), which both entries enforce.
//   grid cap   measured, one MI355X: the 64-bit atomics that end a work-group land on few addresses (the occupied bins; the two
//              counts) and serialise there, about 14 ns each, while all work-groups end together.  At 2^24 pairs the histogram
//              took 49 / 35 / 31 us with at most 2048 / 1024 / 512 work-groups (Gaussian noise) and at 2^27 pairs 190 / 177 /
//              236 us (512: too few loads in flight); the quantiser with both counts non-zero everywhere 44 / 36 / 32 us and
//              318 / 292 / 297 us.  Hence 1024 for both.
//   quantize   iq_cf32_quantize_kernel: four pairs per lane, grid-stride: two 16-byte loads, eight multiplies (v_mul_f32: one
//              correctly rounded product), eight v_rndne_f32, compare, clamp, convert, one 16-byte store; the last pairs (fewer
//              than four) one by one.  Loads and stores are the unaligned vector accesses of iq_mix.h's loader (the input is
//              aligned to 8 bytes, the output to 4).  The two counts run per lane in uint32 (a lane sees at most 2^21 pairs), then
//              across the wave by shuffles and across the four waves through LDS; lanes 0 and 1 add a nonzero count to counts[]
//              with one 64-bit global atomic each.  The gain's range keeps a denormal's product below 0.5 (mdc.h), so the result does not
//              depend on the denormal mode the kernel runs in.
// Both calls only enqueue; vector memory for every store and atomic.
#include "mdc_internal.h"

namespace mdc {

namespace {

constexpr int kCfThreads = 256;
constexpr long kCfGridCap = 1024;            // work-groups; beyond it the kernels stride (_cabi.CF32_GRID_CAP; file head)
constexpr int kCfGroupPairs = 1024;          // pairs a work-group takes per stride step (_cabi.CF32_GROUP_PAIRS)
constexpr int kCfReplicas = 16;              // LDS histograms per work-group
constexpr int kCfHistLoads = kCfGroupPairs / (2 * kCfThreads);      // 16-byte loads per lane and step of the histogram
constexpr int64_t kCfMaxPairs = (int64_t)1 << 40;      // (_cabi.CF32_MAX_PAIRS; file head: the uint32 counters)
constexpr float kCfMinGain = 0x1p-126f, kCfMaxGain = 0x1p125f;

typedef unsigned long long u64;

__device__ __forceinline__ void cf_count(unsigned* __restrict__ h, unsigned rep, unsigned bits) {
    atomicAdd(&h[(((bits >> 23) & 0xFFu) << 4) | rep], 1u);      // result unused: ds_add_u32
}

__device__ __forceinline__ void cf_count4(unsigned* __restrict__ h, unsigned rep, const uint4& g) {
    cf_count(h, rep, g.x);
    cf_count(h, rep, g.y);
    cf_count(h, rep, g.z);
    cf_count(h, rep, g.w);
}

__global__ __launch_bounds__(kCfThreads) void iq_cf32_histogram_kernel(const unsigned* __restrict__ iq, long pairs, u64* __restrict__ hist) {
    static_assert(kCfReplicas == 16 && kCfThreads == 256, "word = bin * 16 + replica; one lane per bin at the flush");
    __shared__ unsigned h[256 * kCfReplicas];
    const int tid = threadIdx.x;
    for (int i = tid; i < 256 * kCfReplicas; i += kCfThreads) h[i] = 0;
    __syncthreads();
    const unsigned rep = (unsigned)tid & (kCfReplicas - 1);
    // iq is 8-byte aligned: one pair, or none, lies in front of the first 16-byte boundary
    const long head = (reinterpret_cast<unsigned long>(iq) & 8ul) != 0 && pairs > 0 ? 1 : 0;
    const long groups = (pairs - head) / 2;      // whole 16-byte groups of two pairs
    const uint4* __restrict__ body = reinterpret_cast<const uint4*>(iq + 2 * head);
    constexpr long kStep = kCfGroupPairs / 2;      // groups per work-group and step: kCfHistLoads per lane, kCfThreads apart
    for (long base = (long)blockIdx.x * kStep; base < groups; base += (long)gridDim.x * kStep) {
        if (base + kStep <= groups) {
            uint4 g[kCfHistLoads];
#pragma unroll
            for (int k = 0; k < kCfHistLoads; ++k) g[k] = body[base + k * kCfThreads + tid];
#pragma unroll
            for (int k = 0; k < kCfHistLoads; ++k) cf_count4(h, rep, g[k]);
        } else {
#pragma unroll
            for (int k = 0; k < kCfHistLoads; ++k)
                if (base + k * kCfThreads + tid < groups) cf_count4(h, rep, body[base + k * kCfThreads + tid]);
        }
    }
    if (blockIdx.x == 0) {
        if (tid == 0 && head) {
            const uint2 v = *reinterpret_cast<const uint2*>(iq);
            cf_count(h, rep, v.x);
            cf_count(h, rep, v.y);
        }
        if (tid == 1 && head + 2 * groups < pairs) {      // the tail: the capture's last pair
            const uint2 v = *reinterpret_cast<const uint2*>(iq + 2 * (pairs - 1));
            cf_count(h, rep, v.x);
            cf_count(h, rep, v.y);
        }
    }
    __syncthreads();
    u64 s = 0;
#pragma unroll
    for (int k = 0; k < kCfReplicas; ++k) s += h[tid * kCfReplicas + ((k + tid) & (kCfReplicas - 1))];
    if (s != 0) atomicAdd(&hist[tid], s);
}

// one pair: the packed int16 pair, and the two counts
__device__ __forceinline__ unsigned cf_quantize_pair(unsigned xb, unsigned yb, float gain, unsigned& nonfinite, unsigned& clipped) {
    const bool bad = (xb & 0x7F800000u) == 0x7F800000u || (yb & 0x7F800000u) == 0x7F800000u;
    const float ri = rintf(__uint_as_float(xb) * gain), rq = rintf(__uint_as_float(yb) * gain);
    const int oi = (int)fminf(fmaxf(ri, -32768.0f), 32767.0f), oq = (int)fminf(fmaxf(rq, -32768.0f), 32767.0f);
    nonfinite += bad ? 1u : 0u;
    clipped += !bad && (ri > 32767.0f || ri < -32768.0f) ? 1u : 0u;
    clipped += !bad && (rq > 32767.0f || rq < -32768.0f) ? 1u : 0u;
    return bad ? 0u : ((unsigned)oi & 0xFFFFu) | ((unsigned)oq << 16);
}

__global__ __launch_bounds__(kCfThreads) void iq_cf32_quantize_kernel(const unsigned* __restrict__ iq, long pairs, float gain,
                                                                      unsigned* __restrict__ out, u64* __restrict__ counts) {
    __shared__ unsigned part[kCfThreads / 64][2];
    unsigned nonfinite = 0, clipped = 0;
    const long stride = (long)gridDim.x * kCfGroupPairs;
    for (long n = ((long)blockIdx.x * kCfThreads + threadIdx.x) * 4; n < pairs; n += stride) {
        if (n + 4 <= pairs) {
            uint4 a, b;
            __builtin_memcpy(&a, iq + 2 * n, sizeof(a));
            __builtin_memcpy(&b, iq + 2 * n + 4, sizeof(b));
            const uint4 v = make_uint4(cf_quantize_pair(a.x, a.y, gain, nonfinite, clipped), cf_quantize_pair(a.z, a.w, gain, nonfinite, clipped),
                                       cf_quantize_pair(b.x, b.y, gain, nonfinite, clipped), cf_quantize_pair(b.z, b.w, gain, nonfinite, clipped));
            __builtin_memcpy(out + n, &v, sizeof(v));
        } else {
            for (long m = n; m < pairs; ++m) {
                const uint2 v = *reinterpret_cast<const uint2*>(iq + 2 * m);
                out[m] = cf_quantize_pair(v.x, v.y, gain, nonfinite, clipped);
            }
        }
    }
    if (counts == nullptr) return;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        nonfinite += __shfl_xor(nonfinite, d, 64);
        clipped += __shfl_xor(clipped, d, 64);
    }
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) {
        part[tid >> 6][0] = nonfinite;
        part[tid >> 6][1] = clipped;
    }
    __syncthreads();
    if (tid < 2) {
        const u64 s = (u64)part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
        if (s != 0) atomicAdd(&counts[tid], s);
    }
}

int cf_pairs_check(const char* who, int64_t pairs) {
    if (pairs < 0) { set_error("%s: negative pair count", who); return MDC_EINVAL; }
    if (pairs > kCfMaxPairs) {
        set_error("%s: at most 2^40 pairs per call (got %lld): the work-groups count in 32 bits", who, (long long)pairs);
        return MDC_EINVAL;
    }
    return MDC_OK;
}

unsigned cf_grid(int64_t pairs) {
    const int64_t groups = (pairs + kCfGroupPairs - 1) / kCfGroupPairs;
    return (unsigned)(groups < kCfGridCap ? groups : kCfGridCap);
}

}  // namespace

}  // namespace mdc

using namespace mdc;

int mdc_iq_cf32_histogram(const float* iq_dev, int64_t pairs_in, uint64_t* hist_dev, void* hip_stream) {
    int rc = cf_pairs_check("mdc_iq_cf32_histogram", pairs_in);
    if (rc != MDC_OK) return rc;
    if ((rc = iq_aligned("mdc_iq_cf32_histogram", "iq_dev", iq_dev, 8)) != MDC_OK) return rc;
    if ((rc = iq_aligned("mdc_iq_cf32_histogram", "hist_dev", hist_dev, 8)) != MDC_OK) return rc;
    if (pairs_in == 0) return MDC_OK;
    if (!iq_dev || !hist_dev) { set_error("mdc_iq_cf32_histogram: null buffer"); return MDC_EINVAL; }
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return guarded("mdc_iq_cf32_histogram", [&]() -> int {
        hipLaunchKernelGGL(iq_cf32_histogram_kernel, dim3(cf_grid(pairs_in)), dim3(kCfThreads), 0, s,
                           reinterpret_cast<const unsigned*>(iq_dev), (long)pairs_in, reinterpret_cast<u64*>(hist_dev));
        MDC_HIP(hipGetLastError());
        return MDC_OK;
    });
}

int mdc_iq_cf32_quantize(const float* iq_dev, int64_t pairs_in, float gain, int16_t* out_dev, uint64_t* counts_dev, void* hip_stream) {
    int rc = cf_pairs_check("mdc_iq_cf32_quantize", pairs_in);
    if (rc != MDC_OK) return rc;
    if (!(gain >= kCfMinGain && gain <= kCfMaxGain)) {      // (a NaN fails both comparisons)
        set_error("mdc_iq_cf32_quantize: gain must be finite and in 2^-126 .. 2^125 (got %g)", (double)gain);
        return MDC_EINVAL;
    }
    if ((rc = iq_aligned("mdc_iq_cf32_quantize", "iq_dev", iq_dev, 8)) != MDC_OK) return rc;
    if ((rc = iq_aligned("mdc_iq_cf32_quantize", "output", out_dev, 4)) != MDC_OK) return rc;
    if ((rc = iq_aligned("mdc_iq_cf32_quantize", "counts_dev", counts_dev, 8)) != MDC_OK) return rc;
    if (pairs_in == 0) return MDC_OK;
    if (!iq_dev || !out_dev) { set_error("mdc_iq_cf32_quantize: null buffer"); return MDC_EINVAL; }
    const uintptr_t in0 = reinterpret_cast<uintptr_t>(iq_dev), out0 = reinterpret_cast<uintptr_t>(out_dev);
    const uintptr_t in_bytes = (uintptr_t)pairs_in * 8, out_bytes = (uintptr_t)pairs_in * 4;
    if (in0 < out0 + out_bytes && out0 < in0 + in_bytes) { set_error("mdc_iq_cf32_quantize: output must not overlap the input"); return MDC_EINVAL; }
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return guarded("mdc_iq_cf32_quantize", [&]() -> int {
        hipLaunchKernelGGL(iq_cf32_quantize_kernel, dim3(cf_grid(pairs_in)), dim3(kCfThreads), 0, s,
                           reinterpret_cast<const unsigned*>(iq_dev), (long)pairs_in, gain, reinterpret_cast<unsigned*>(out_dev), reinterpret_cast<u64*>(counts_dev));
        MDC_HIP(hipGetLastError());
        return MDC_OK;
    });
}
