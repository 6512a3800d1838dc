// The host side of the rational resampler's geometry -- limits, tiling, the branch-major tap image -- for the two kernels that
// use it: mdc_iq_resample (iq_resample.hip, which describes all of it at its head) and mdc_iq_extract (iq_extract.hip).
// Everything here has internal linkage.
#pragma once
#include "iq_mix.h"

namespace mdc {

namespace {

constexpr int kResThreads = kIqMixThreads;
constexpr long kResGridCap = 1024;       // work-groups; beyond it the kernel strides (_cabi.RESAMPLE_GRID_CAP)
constexpr int kResMaxTaps = 1024, kResMaxDecimate = 256, kResMaxInterpolate = 32;
constexpr int kResTapGroup = 4;          // tap dwords per step of the filter loop
constexpr int kResTapDwords = 768;       // the branch-major image: L * stride <= 651 dwords over all 1 <= L <= 32, T <= 1024

struct ResTaps { unsigned pk[kResTapDwords]; };

struct ResPlan {
    int L, D, ngroups, stride, tapdw, tile_out, tile_in;
    bool odd;
};

int64_t resample_out_count(int64_t pairs, int ntaps, int L, int D) {
    if (pairs < 1) return 0;
    const int64_t lv = (pairs - 1) * L + 1;      // the zero-stuffed length; pairs <= 2^58 is checked
    return iq_span_count(lv, ntaps, D);
}

int resample_shape_check(const char* who, int64_t pairs, int ntaps, int L, int D) {
    if (L < 1 || L > kResMaxInterpolate) { set_error("%s: interpolate must be in 1..%d (got %d)", who, kResMaxInterpolate, L); return MDC_EINVAL; }
    if (D < 1 || D > kResMaxDecimate) { set_error("%s: decimate must be in 1..%d (got %d)", who, kResMaxDecimate, D); return MDC_EINVAL; }
    if (ntaps < 1 || ntaps > kResMaxTaps) { set_error("%s: ntaps must be in 1..%d (got %d)", who, kResMaxTaps, ntaps); return MDC_EINVAL; }
    if (pairs < 0) { set_error("%s: negative pair count", who); return MDC_EINVAL; }
    if (pairs > ((int64_t)1 << 58)) { set_error("%s: pair count beyond 2^58", who); return MDC_EINVAL; }
    return MDC_OK;
}

int gcd(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

// the tiling for (L, D, ntaps); false if the tap image does not fit (it always does: see kResTapDwords)
bool resample_geometry(int L, int D, int ntaps, ResPlan& p) {
    const int longest = (ntaps + L - 1) / L;                                     // taps of branch 0, the longest branch
    p.L = L;
    p.D = D;
    p.ngroups = ((longest + 1) / 2 + kResTapGroup - 1) / kResTapGroup;
    p.stride = (kResTapGroup * p.ngroups) | 1;
    p.tapdw = L * p.stride;
    if (p.tapdw > kResTapDwords) return false;
    const int q = (kIqTilePairs - longest) / D;                                  // >= (8192 - 1024) / 256
    p.tile_out = q * L;
    p.tile_in = q * D;
    // an output of the class c (mod L / g) of a tile starts at the local sample ceil(c D / L) + k D / g
    const int g = gcd(L, D);
    p.odd = ((D / g) & 1) != 0;
    for (int c = 0; c < L / g && !p.odd; ++c) p.odd = (((c * D + L - 1) / L) & 1) != 0;
    return true;
}

// the tiling and the branch-major tap image (pk: p.tapdw dwords, zero on entry) for (L, D, taps)
bool resample_plan(int L, int D, const int16_t* h, int ntaps, ResPlan& p, unsigned* pk) {
    if (!resample_geometry(L, D, ntaps, p)) return false;
    for (int r = 0; r < L; ++r)
        for (int i = 0; r + i * L < ntaps; ++i) pk[r * p.stride + (i >> 1)] |= (unsigned)(uint16_t)h[r + i * L] << (16 * (i & 1));
    return true;
}

// 0, or 1 + the first branch r whose sum_i |h[r + i L]| exceeds 65535 (*sum: that branch's sum)
int resample_branch_over(const int16_t* h, int ntaps, int L, long* sum) {
    for (int r = 0; r < L && r < ntaps; ++r) {
        long abs_sum = 0;
        for (int k = r; k < ntaps; k += L) abs_sum += h[k] < 0 ? -(long)h[k] : (long)h[k];
        if (abs_sum > 65535) { *sum = abs_sum; return r + 1; }
    }
    return 0;
}

}  // namespace

}  // namespace mdc
