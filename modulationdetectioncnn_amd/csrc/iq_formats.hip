// mdc_iq_windows / mdc_iq_windows_norm -- the raw-I/Q front-end per sample format: unsigned 8-bit (RTL-SDR, SigMF cu8), signed
// 8-bit (HackRF, SigMF ci8) and signed 16-bit little-endian (USRP sc16, SDRplay, bladeRF, Airspy, SigMF ci16_le) captures.  The
// wave-per-window normaliser of all three lives here, mdc_iq_u8_windows_norm's included (iq_norm.hip keeps that entry's other
// kernel); it writes the statistics as the 64-bit record mdc_iq_window_stats64 or, for MDC_IQ_CU8 alone, as the 32-bit
// mdc_iq_window_stats (include/mdc.h).  Plain MDC_IQ_CU8 conversion goes to iq_u8_launch (eval_ops.hip).
//
// One wave per window; lane l holds the window's pairs 2l and 2l+1 = (I0, Q0, I1, Q1): 4 bytes (8-bit formats) or 8 bytes
// (CI16), loaded with one unaligned vector load (a window at an odd hop starts on a pair, no better).  Everything up to the
// energy is integer arithmetic.  For int16 no "fits 32 bits" argument holds: the four squares of ONE lane can sum to 2^32, the
// wave's to 2^38, E reaches 2^45.  What is summed over the wave is therefore kept in pieces that provably fit 32 bits:
//     CU8    three byte sums on the raw bytes b (s = 2 b - 255 is never formed per sample for the sums): sum_I b, sum_Q b (one
//            v_dot4_u32_u8 each against the byte masks 0x00010001 / 0x01000100; both <= 32,640: the two halves of ONE
//            register for the reduction), sum b^2 (one v_dot4_u32_u8 of the word with itself)        -- 2 reductions
//     CI8    the same three sums on b = s + 128 (the bytes with their sign bits flipped), sum b^2 < 2^24 -- 2 reductions
//     CI16   I0 + I1 + 2^16 and Q0 + Q1 + 2^16 (lane <= 2^17, wave <= 2^23); the squares as a = I0^2 + Q0^2, b = I1^2 + Q1^2
//            (each <= 2^31, as unsigned) split into (a & 0xFFFF) + (b & 0xFFFF) (wave < 2^23) and (a >> 16) + (b >> 16)
//            (wave <= 2^22), recombined in 64 bits                                                   -- 4 reductions
// A reduction is four DPP row steps (quad swaps, half-row mirror, row mirror: no LDS) and four v_readlane of the row sums: the
// totals arrive in scalar registers, and the record (sum_i^2 needs 64 bits; E = 128 sum_sq - sum_i^2 - sum_q^2 is formed in
// uint64, where 128 sum_sq <= 2^45 and every partial difference is >= 0 by Cauchy-Schwarz) is scalar arithmetic.  For CU8 every
// field is below 2^31 (window_stats, iq_norm.hip): the 32-bit record is the same integers, narrowed.
// Frames: the centred sample times 128, 128 s - c, is an integer below 2^23: exact in f32.  x = (float)(128 s - c) * (level /
// sqrtf((float)E)) is then one correctly rounded conversion of the 64-bit integer E, one square root, one division and one
// multiplication, each correctly rounded (hipcc's default for f32 sqrt and division) -- tests/test_iq_norm_gpu.py derives its
// 2^-21 relative bound from exactly these.
// A wave takes two ADJACENT windows per step and a work-group 2 * kFmtWaves consecutive ones, so both loads are in flight
// together, the frames leave as one contiguous 8 KiB run per work-group step, and with a small hop the windows' common bytes
// come from the CU's L1 after their first read.
// Vector memory only.
#include "mdc_internal.h"

namespace mdc {

namespace {

constexpr int kFmtWaves = 4;

template <int FMT> struct LaneWord { using type = unsigned; static constexpr int kPairBytes = 2; };
template <> struct LaneWord<MDC_IQ_CI16> { using type = uint2; static constexpr int kPairBytes = 4; };

template <int FMT>
__device__ __forceinline__ typename LaneWord<FMT>::type load_lane(const unsigned char* p) {      // one global_load_dword / dwordx2
    typename LaneWord<FMT>::type r;
    __builtin_memcpy(&r, p, sizeof(r));
    return r;
}

// the lane's four integer samples s: (I0, Q0, I1, Q1)
template <int FMT> __device__ __forceinline__ int4 lane_samples(unsigned w) {
    if (FMT == MDC_IQ_CU8)
        return make_int4(2 * (int)(w & 0xFFu) - 255, 2 * (int)((w >> 8) & 0xFFu) - 255, 2 * (int)((w >> 16) & 0xFFu) - 255, 2 * (int)(w >> 24) - 255);
    return make_int4((int)(signed char)(w & 0xFFu), (int)(signed char)((w >> 8) & 0xFFu), (int)(signed char)((w >> 16) & 0xFFu),
                     (int)(signed char)(w >> 24));
}
template <int FMT> __device__ __forceinline__ int4 lane_samples(uint2 w) {
    return make_int4((int)(short)(w.x & 0xFFFFu), (int)(short)(w.x >> 16), (int)(short)(w.y & 0xFFFFu), (int)(short)(w.y >> 16));
}

template <int CTRL> __device__ __forceinline__ unsigned dpp_add(unsigned v) {
    return v + (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
// sum over the 64 lanes (all active), uniform: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror leave
// every lane with its row's sum; the four rows are added from one lane each
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
    v = dpp_add<0xB1>(v);
    v = dpp_add<0x4E>(v);
    v = dpp_add<0x141>(v);
    v = dpp_add<0x140>(v);
    return (unsigned)__builtin_amdgcn_readlane((int)v, 0) + (unsigned)__builtin_amdgcn_readlane((int)v, 16) +
           (unsigned)__builtin_amdgcn_readlane((int)v, 32) + (unsigned)__builtin_amdgcn_readlane((int)v, 48);
}

struct WindowSums { long long sum_i, sum_q; unsigned long long sum_sq; };

// 8-bit formats: the byte sums on the unsigned bytes b (CU8: s = 2 b - 255; CI8: s = b - 128 after the flip)
template <int FMT> __device__ __forceinline__ WindowSums window_sums(unsigned w) {
    if (FMT == MDC_IQ_CI8) w ^= 0x80808080u;
    const unsigned bi = __builtin_amdgcn_udot4(w, 0x00010001u, 0u, false);
    const unsigned bq = __builtin_amdgcn_udot4(w, 0x01000100u, 0u, false);
    const unsigned iq = wave_sum(bi | (bq << 16));
    const unsigned b2 = wave_sum(__builtin_amdgcn_udot4(w, w, 0u, false));
    const unsigned sbi = iq & 0xFFFFu, sbq = iq >> 16;
    WindowSums r;
    if (FMT == MDC_IQ_CU8) {
        r.sum_i = (int)(2u * sbi) - 32640;
        r.sum_q = (int)(2u * sbq) - 32640;
        r.sum_sq = 4u * b2 - 1020u * (sbi + sbq) + 255u * 255u * 256u;      // (mod 2^32; the value is <= 16,646,400)
    } else {
        r.sum_i = (int)sbi - 128 * 128;
        r.sum_q = (int)sbq - 128 * 128;
        r.sum_sq = b2 - 256u * (sbi + sbq) + 256u * 128u * 128u;            // sum (b - 128)^2 over 256 samples, <= 2^22
    }
    return r;
}
template <int FMT> __device__ __forceinline__ WindowSums window_sums(uint2 w) {
    const int4 s = lane_samples<FMT>(w);
    const unsigned bi = wave_sum((unsigned)(s.x + s.z + 65536)), bq = wave_sum((unsigned)(s.y + s.w + 65536));
    const unsigned a = (unsigned)(s.x * s.x) + (unsigned)(s.y * s.y), b = (unsigned)(s.z * s.z) + (unsigned)(s.w * s.w);      // each <= 2^31
    const unsigned lo = wave_sum((a & 0xFFFFu) + (b & 0xFFFFu)), hi = wave_sum((a >> 16) + (b >> 16));
    WindowSums r;
    r.sum_i = (long long)bi - 64ll * 65536ll;
    r.sum_q = (long long)bq - 64ll * 65536ll;
    r.sum_sq = ((unsigned long long)hi << 16) + lo;
    return r;
}

__device__ __forceinline__ void store_record(mdc_iq_window_stats64* rec, const WindowSums& t, unsigned long long energy) {
    ulonglong2* r = reinterpret_cast<ulonglong2*>(rec);
    r[0] = make_ulonglong2((unsigned long long)t.sum_i, (unsigned long long)t.sum_q);
    r[1] = make_ulonglong2(t.sum_sq, energy);
}
__device__ __forceinline__ void store_record(mdc_iq_window_stats* rec, const WindowSums& t, unsigned long long energy) {      // CU8 only
    *reinterpret_cast<int4*>(rec) = make_int4((int)t.sum_i, (int)t.sum_q, (int)t.sum_sq, (int)energy);
}

// the whole window's work for one wave; w = this lane's two pairs.  REC: the record written (void: none)
template <int FMT, bool FRAMES, class REC>
__device__ __forceinline__ void norm_window(typename LaneWord<FMT>::type w, long f, int lane, bool remove_dc, float level, float* __restrict__ x,
                                            REC* __restrict__ stats) {
    const WindowSums t = window_sums<FMT>(w);
    // uint64: 128 sum_sq <= 2^45; 128 sum_sq - sum_i^2 >= sum_q^2 >= 0, so neither subtraction wraps
    unsigned long long energy = 128ull * t.sum_sq;
    if (remove_dc) {
        energy -= (unsigned long long)(t.sum_i * t.sum_i);
        energy -= (unsigned long long)(t.sum_q * t.sum_q);
    }
    if constexpr (!std::is_void<REC>::value) {
        if (lane == 0) store_record(stats + f, t, energy);
    }
    if (FRAMES) {
        const float g = energy ? level / sqrtf((float)energy) : 0.f;      // a constant window (E = 0): zeros, never 0 / 0
        const int ci = remove_dc ? (int)t.sum_i : 0, cq = remove_dc ? (int)t.sum_q : 0;
        const int4 s = lane_samples<FMT>(w);
        float* row_i = x + f * kFrameFloats + 2 * lane;
        *reinterpret_cast<float2*>(row_i) = make_float2((float)(128 * s.x - ci) * g, (float)(128 * s.z - ci) * g);
        *reinterpret_cast<float2*>(row_i + kSamples) = make_float2((float)(128 * s.y - cq) * g, (float)(128 * s.w - cq) * g);
    }
}

// two ADJACENT windows per wave and step, 2 * kFmtWaves consecutive ones per work-group
template <int FMT, bool FRAMES, class REC>
__global__ __launch_bounds__(64 * kFmtWaves) void iq_fmt_norm_kernel(const unsigned char* __restrict__ iq, long n, long hop_bytes, float level,
                                                                    int remove_dc, float* __restrict__ x, REC* __restrict__ stats) {
    constexpr int kLaneBytes = 2 * LaneWord<FMT>::kPairBytes;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // (scalar loop control)
    const long step = (long)gridDim.x * (2 * kFmtWaves);
    // f0 is uniform over the wave: the reductions see all 64 lanes of one window; windows past n are never read or written
    for (long f0 = (long)blockIdx.x * (2 * kFmtWaves) + 2 * wave; f0 < n; f0 += step) {
        const bool two = f0 + 1 < n;
        const auto w0 = load_lane<FMT>(iq + hop_bytes * f0 + kLaneBytes * lane);
        auto w1 = w0;
        if (two) w1 = load_lane<FMT>(iq + hop_bytes * (f0 + 1) + kLaneBytes * lane);
        norm_window<FMT, FRAMES, REC>(w0, f0, lane, remove_dc != 0, level, x, stats);
        if (two) norm_window<FMT, FRAMES, REC>(w1, f0 + 1, lane, remove_dc != 0, level, x, stats);
    }
}

// mdc_iq_windows for the signed formats: x = (float)s * scale, the window's two rows from the same lane layout
template <int FMT>
__global__ __launch_bounds__(64 * kFmtWaves) void iq_fmt_convert_kernel(const unsigned char* __restrict__ iq, long n, long hop_bytes, float scale,
                                                                       float* __restrict__ x) {
    constexpr int kLaneBytes = 2 * LaneWord<FMT>::kPairBytes;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long f = (long)blockIdx.x * kFmtWaves + wave; f < n; f += (long)gridDim.x * kFmtWaves) {
        const int4 s = lane_samples<FMT>(load_lane<FMT>(iq + hop_bytes * f + kLaneBytes * lane));
        float* row_i = x + f * kFrameFloats + 2 * lane;
        *reinterpret_cast<float2*>(row_i) = make_float2((float)s.x * scale, (float)s.z * scale);
        *reinterpret_cast<float2*>(row_i + kSamples) = make_float2((float)s.y * scale, (float)s.w * scale);
    }
}

template <int FMT, class REC>
int norm_launch(const unsigned char* iq, int64_t n, int64_t hop, float level, int flags, float* x, REC* stats, hipStream_t s) {
    long grid = (n + 2 * kFmtWaves - 1) / (2 * kFmtWaves);
    if (grid > kIqGridCap) grid = kIqGridCap;
    const dim3 g((unsigned)grid), b(64 * kFmtWaves);
    const long hop_bytes = (long)hop * LaneWord<FMT>::kPairBytes;
    const int dc = (flags & MDC_IQ_REMOVE_DC) != 0;
    if (x && stats) hipLaunchKernelGGL((iq_fmt_norm_kernel<FMT, true, REC>), g, b, 0, s, iq, (long)n, hop_bytes, level, dc, x, stats);
    else if (x)     hipLaunchKernelGGL((iq_fmt_norm_kernel<FMT, true, void>), g, b, 0, s, iq, (long)n, hop_bytes, level, dc, x, (void*)nullptr);
    else            hipLaunchKernelGGL((iq_fmt_norm_kernel<FMT, false, REC>), g, b, 0, s, iq, (long)n, hop_bytes, level, dc, x, stats);
    MDC_HIP(hipGetLastError());
    return MDC_OK;
}

template <int FMT>
int convert_launch(const unsigned char* iq, int64_t n, int64_t hop, float scale, float* x, hipStream_t s) {
    long grid = (n + kFmtWaves - 1) / kFmtWaves;
    if (grid > kIqGridCap) grid = kIqGridCap;
    hipLaunchKernelGGL(iq_fmt_convert_kernel<FMT>, dim3((unsigned)grid), dim3(64 * kFmtWaves), 0, s, iq, (long)n,
                       (long)hop * LaneWord<FMT>::kPairBytes, scale, x);
    MDC_HIP(hipGetLastError());
    return MDC_OK;
}

}  // namespace

int iq_pair_bytes(int format) { return format == MDC_IQ_CI16 ? 4 : (format == MDC_IQ_CU8 || format == MDC_IQ_CI8) ? 2 : 0; }

int iq_format_known(const char* who, int format) {
    if (iq_pair_bytes(format) != 0) return MDC_OK;
    set_error("%s: unknown sample format %d (MDC_IQ_CU8, MDC_IQ_CI8, MDC_IQ_CI16)", who, format);
    return MDC_EINVAL;
}

int iq_pair_aligned(const char* who, const char* what, int format, const void* p) {
    const int pair_bytes = iq_pair_bytes(format);
    if ((reinterpret_cast<uintptr_t>(p) & (uintptr_t)(pair_bytes - 1)) == 0) return MDC_OK;
    set_error("%s: %s must start on a whole (I,Q) pair (%d-byte aligned)", who, what, pair_bytes);
    return MDC_EINVAL;
}

int iq_aligned(const char* who, const char* what, const void* p, int bytes) {
    if ((reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) == 0) return MDC_OK;
    set_error("%s: %s must be %d-byte aligned", who, what, bytes);
    return MDC_EINVAL;
}

int iq_format_check(const char* who, int format, int64_t hop) {
    const int rc = iq_format_known(who, format);
    if (rc != MDC_OK) return rc;
    if (hop < 1 || hop > (int64_t)1 << 24) { set_error("%s: hop must be in 1..2^24 sample pairs (got %lld)", who, (long long)hop); return MDC_EINVAL; }
    return MDC_OK;
}

int iq_norm_wave_launch(const uint8_t* iq, int64_t n, int64_t hop, float level, int flags, float* x, mdc_iq_window_stats* stats, hipStream_t s) {
    return norm_launch<MDC_IQ_CU8>(iq, n, hop, level, flags, x, stats, s);
}

}  // namespace mdc

using namespace mdc;

int mdc_iq_windows(const void* iq_dev, int format, int64_t n, int64_t hop, float scale, float* x_dev, void* hip_stream) {
    if (n < 0) { set_error("mdc_iq_windows: negative window count"); return MDC_EINVAL; }
    int rc = iq_format_check("mdc_iq_windows", format, hop);
    if (rc != MDC_OK) return rc;
    if (n == 0) return MDC_OK;
    if (!iq_dev || !x_dev) { set_error("mdc_iq_windows: null buffer"); return MDC_EINVAL; }
    if ((reinterpret_cast<uintptr_t>(x_dev) & 7) != 0) { set_error("mdc_iq_windows: frames must be 8-byte aligned"); return MDC_EINVAL; }
    if ((rc = iq_pair_aligned("mdc_iq_windows", "input", format, iq_dev)) != MDC_OK) return rc;
    const unsigned char* p = static_cast<const unsigned char*>(iq_dev);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return guarded("mdc_iq_windows", [&]() -> int {
        return with_format(format, [&](auto fmt) {
            if constexpr (decltype(fmt)::value == MDC_IQ_CU8) return iq_u8_launch(p, n, hop, scale, x_dev, s);
            else return convert_launch<decltype(fmt)::value>(p, n, hop, scale, x_dev, s);
        });
    });
}

int mdc_iq_windows_norm(const void* iq_dev, int format, int64_t n, int64_t hop, float level, int flags, float* x_dev,
                        mdc_iq_window_stats64* stats64_dev, void* hip_stream) {
    if (n < 0) { set_error("mdc_iq_windows_norm: negative window count"); return MDC_EINVAL; }
    int rc = iq_format_check("mdc_iq_windows_norm", format, hop);
    if (rc != MDC_OK) return rc;
    if ((rc = iq_norm_check("mdc_iq_windows_norm", hop, level, flags)) != MDC_OK) return rc;
    if (n == 0) return MDC_OK;
    if (!x_dev && !stats64_dev) { set_error("mdc_iq_windows_norm: null buffer: x_dev and stats64_dev are both null (nothing to compute)"); return MDC_EINVAL; }
    if ((reinterpret_cast<uintptr_t>(x_dev) & 7) != 0) { set_error("mdc_iq_windows_norm: frames must be 8-byte aligned"); return MDC_EINVAL; }
    if ((reinterpret_cast<uintptr_t>(stats64_dev) & 15) != 0) { set_error("mdc_iq_windows_norm: statistics must be 16-byte aligned"); return MDC_EINVAL; }
    if (!iq_dev) { set_error("mdc_iq_windows_norm: null buffer (iq_dev)"); return MDC_EINVAL; }
    if ((rc = iq_pair_aligned("mdc_iq_windows_norm", "input", format, iq_dev)) != MDC_OK) return rc;
    const unsigned char* p = static_cast<const unsigned char*>(iq_dev);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return guarded("mdc_iq_windows_norm", [&]() -> int {
        return with_format(format, [&](auto fmt) { return norm_launch<decltype(fmt)::value>(p, n, hop, level, flags, x_dev, stats64_dev, s); });
    });
}
