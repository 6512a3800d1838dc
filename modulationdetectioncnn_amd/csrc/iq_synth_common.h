// What mdc_iq_synth_frames (iq_synth.hip) and mdc_iq_synth_capture (iq_synth_capture.hip) share: the plan blob's records and limits,
// the counter-based draws of include/mdc.h ("frame synthesis": k_seed, key_f, d(j), g()) and the check a run call makes of a plan
// blob before a kernel reads what its records name.  One copy, so the two definitions cannot drift apart.
// Everything here has internal linkage.
#pragma once
#include "iq_mix.h"
#include "mdc_fmix32.h"

#include <cstring>

namespace mdc {

namespace {

constexpr uint32_t kSynMagic = 0x5953434Du;      // "MCSY"
constexpr uint32_t kSynVersion = 1;
constexpr int kSynMaxClasses = 64, kSynMaxSnrs = 64, kSynMaxPoints = 64;
constexpr int kSynMaxSps = 16, kSynMaxSpan = 16, kSynMaxTaps = 128;
constexpr int kSynGaussMax = 262140;             // |sum of eight uint16 - 4 * 65535|
constexpr uint32_t kSynMaxStep = 1u << 30;
constexpr int kSynMaxQ = 40;
constexpr unsigned kSynDrawStride = 0xC2B2AE35u;
constexpr unsigned kSynDrawSymbols = 16, kSynDrawNoise = 1024;

typedef unsigned long long u64;

// the blob: SynHeader | classes (SynClass) | alphabets (dwords re | im << 16) | tap images (dwords, branch-major) | gain_sig (int32,
// class-major) | gain_noise (int32); every part starts on a multiple of 16 bytes, all offsets are from the blob's first byte
struct SynHeader {
    uint32_t magic, version;
    int32_t C, S, q;
    uint32_t max_step;
    int64_t bytes, off_classes, off_points, off_taps, off_gsig, off_gnoise;
    int64_t reserved;
};
struct SynClass {
    int32_t source, points, sps, span, mode, factor, amp, add_re, add_im;
    int32_t point0, tap0;      // the class's first dword in the alphabets / in the tap images
    int32_t nsym;              // symbols a frame draws: (127 + sps - 1) / sps + span
};
static_assert(sizeof(SynHeader) == 80 && sizeof(SynClass) == 48 && sizeof(mdc_iq_synth_class) == 40, "the plan blob's records");

__host__ __device__ __forceinline__ unsigned syn_seed_key(u64 seed) {
    return fmix32(fmix32((unsigned)seed + 0x9E3779B9u) ^ (unsigned)(seed >> 32));
}
__host__ __device__ __forceinline__ unsigned syn_frame_key(unsigned kseed, u64 f) {
    return fmix32(fmix32(kseed ^ ((unsigned)f * 0x85EBCA6Bu)) ^ ((unsigned)(f >> 32) * 0x85EBCA6Bu + 1u));
}
__host__ __device__ __forceinline__ unsigned syn_draw(unsigned key, unsigned j) { return fmix32(key + j * kSynDrawStride); }
// the sum of the eight 16-bit halves of draws j .. j + 3, minus 262140
__device__ __forceinline__ int syn_gauss(unsigned key, unsigned j) {
    int s = -kSynGaussMax;
#pragma unroll
    for (unsigned e = 0; e < 4; ++e) {
        const unsigned d = syn_draw(key, j + e);
        s += (int)(d & 0xFFFFu) + (int)(d >> 16);
    }
    return s;
}

inline int64_t round16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// a run call's check of a plan blob, on the host copy: the header, then every class record's indices (the kernels read the
// alphabets and tap images they name); on success h holds the header
inline int syn_plan_open(const char* who, const void* plan_host, int64_t plan_bytes, SynHeader& h) {
    if (!plan_host) { set_error("%s: null plan", who); return MDC_EINVAL; }
    if (plan_bytes < (int64_t)sizeof(SynHeader)) { set_error("%s: plan_bytes is %lld, smaller than a plan's header", who, (long long)plan_bytes); return MDC_EINVAL; }
    memcpy(&h, plan_host, sizeof h);
    if (h.magic != kSynMagic || h.version != kSynVersion) { set_error("%s: plan_host does not hold a plan of mdc_iq_synth_plan", who); return MDC_EINVAL; }
    if (h.bytes != plan_bytes) { set_error("%s: plan_bytes is %lld, the plan holds %lld bytes", who, (long long)plan_bytes, (long long)h.bytes); return MDC_EINVAL; }
    if (h.C < 1 || h.C > kSynMaxClasses || h.S < 1 || h.S > kSynMaxSnrs || h.q < 1 || h.q > kSynMaxQ || h.max_step > kSynMaxStep ||
        h.off_classes != (int64_t)sizeof(SynHeader) || h.off_points != h.off_classes + (int64_t)h.C * (int64_t)sizeof(SynClass) ||
        h.off_taps < h.off_points || (h.off_taps & 15) != 0 || h.off_gsig < h.off_taps || (h.off_gsig & 15) != 0 ||
        h.off_gnoise != round16(h.off_gsig + 4 * (int64_t)h.C * h.S) || h.bytes != round16(h.off_gnoise + 4 * (int64_t)h.S)) {
        set_error("%s: the plan's header is damaged", who);
        return MDC_EINVAL;
    }
    return MDC_OK;
}
inline int syn_plan_classes_check(const char* who, const void* plan_host, const SynHeader& h) {
    const int64_t npoints = (h.off_taps - h.off_points) / 4, ntaps = (h.off_gsig - h.off_taps) / 4;
    for (int32_t k = 0; k < h.C; ++k) {
        SynClass c;
        memcpy(&c, static_cast<const unsigned char*>(plan_host) + h.off_classes + (int64_t)k * (int64_t)sizeof c, sizeof c);
        if (c.sps < 1 || c.sps > kSynMaxSps || c.span < 1 || c.span > kSynMaxSpan || c.sps * c.span > kSynMaxTaps || c.points < 0 ||
            c.points > kSynMaxPoints || (c.source == MDC_SYNTH_ALPHABET && c.points < 1) || c.point0 < 0 || c.point0 + c.points > npoints ||
            c.tap0 < 0 || c.tap0 + c.sps * c.span > ntaps || c.nsym != (kSamples - 1 + c.sps - 1) / c.sps + c.span) {
            set_error("%s: the plan's record of class %d is damaged", who, k);
            return MDC_EINVAL;
        }
    }
    return MDC_OK;
}

}  // namespace

}  // namespace mdc
