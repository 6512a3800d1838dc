// mdc_iq_ddc -- tune, low-pass and decimate a wideband integer I/Q capture on the device, in exact integer arithmetic
// (include/mdc.h, "digital down-converter"; the numpy int64 restatement is tests/iq_ddc_ref.py).  One pass over the capture:
//
//   tile      the capture's outputs are cut into tiles of `tile_out` = (kDdcTilePairs - T) / D + 1 outputs: such a tile reads
//             (tile_out - 1) D + T <= kDdcTilePairs input pairs, its own D tile_out and the T - D pairs of halo.  Work-groups
//             stride over the tiles (grid cap kDdcGridCap).
//   mix       mix_tile of iq_mix.h: quads of pairs -> two planar int16 LDS images (re, im), 33-dword stride.
//   filter    fir_output of iq_mix.h, one lane per output j from the local sample j D on, in groups of 8 tap dwords.  The tap
//             pairs are uniform over the wave -- they are kernel ARGUMENTS (2 KiB by value: no copy to wait for, nothing to
//             allocate, and the compiler reads them with scalar loads), zero-padded to whole groups.  T odd: the last pair's
//             second tap is that padding.  j D odd is only possible for odd D: the ODD instantiations.
// Everything the filter reads beyond the tile's last needed sample (the taps' zero padding times it) is still written by the
// mix step -- zeros beyond the capture -- so the result never depends on stale LDS.
// The call only enqueues; vector memory for every store.  mdc_iq_resample shares the mix stage and the filter.
#include "iq_mix.h"

namespace mdc {

namespace {

constexpr int kDdcThreads = kIqMixThreads;
constexpr int kDdcTilePairs = kIqTilePairs;      // input pairs a tile spans at most: (tile_out - 1) D + T
constexpr long kDdcGridCap = 1024;       // work-groups; beyond it the kernel strides (_cabi.DDC_GRID_CAP)
constexpr int kMaxTaps = 1024, kMaxDecimate = 256;
constexpr int kTapGroup = 8;             // tap dwords per step of the filter loop

const unsigned h_nco[kNcoEntries] = {
#include "iq_ddc_nco_table.h"
};

struct DdcTaps { unsigned pk[kMaxTaps / 2]; };      // pk[i] = h[2i] | h[2i+1] << 16, zeros beyond the taps

template <int FMT, bool ODD>
__global__ __launch_bounds__(kDdcThreads) void iq_ddc_kernel(const unsigned char* __restrict__ iq, long pairs, unsigned phase0, unsigned step,
                                                             int D, int ngroups, int tile_out, long n_out, long ntiles,
                                                             unsigned* __restrict__ out, const DdcTaps taps) {
    __shared__ unsigned lds[kNcoEntries + 2 * kPlaneDwords];
    unsigned* nco = lds;
    unsigned* re = lds + kNcoEntries;
    unsigned* im = re + kPlaneDwords;
    const int tid = threadIdx.x;
    for (int i = tid; i < kNcoEntries; i += kDdcThreads) nco[i] = d_nco[i];

    for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long out0 = t * tile_out, in0 = out0 * D;
        const long left = n_out - out0;
        const int nout = left < tile_out ? (int)left : tile_out;
        // local pairs the filter reads: the last output's start, its tap groups, one more dword for the ODD look-ahead
        const int span = (nout - 1) * D + 2 * kTapGroup * ngroups + 2;      // <= kDdcTilePairs + 17
        const int quads = (span + 3) >> 2;
        __syncthreads();      // the table is in place; the previous tile's filter has read its samples
        mix_tile<FMT>(iq, in0, pairs, phase0, step, quads, nco, re, im, tid);
        __syncthreads();
        for (int j = tid; j < nout; j += kDdcThreads) {
            const int start = j * D, base = start >> 1;
            const unsigned sh = (unsigned)(start & 1) << 4;
            out[out0 + j] = fir_output<ODD, kTapGroup>(re, im, base, sh, ngroups, [&](int k) { return taps.pk[k]; });
        }
    }
}

template <int FMT>
int ddc_launch(const unsigned char* iq, int64_t pairs, uint32_t phase0, uint32_t step, int D, int ngroups, int tile_out, int64_t n_out,
               int16_t* out, const DdcTaps& taps, hipStream_t s) {
    const long ntiles = (n_out + tile_out - 1) / tile_out;
    const dim3 g((unsigned)(ntiles < kDdcGridCap ? ntiles : kDdcGridCap)), b(kDdcThreads);
    unsigned* o = reinterpret_cast<unsigned*>(out);
    if (D & 1) hipLaunchKernelGGL((iq_ddc_kernel<FMT, true>), g, b, 0, s, iq, (long)pairs, phase0, step, D, ngroups, tile_out, (long)n_out, ntiles, o, taps);
    else       hipLaunchKernelGGL((iq_ddc_kernel<FMT, false>), g, b, 0, s, iq, (long)pairs, phase0, step, D, ngroups, tile_out, (long)n_out, ntiles, o, taps);
    MDC_HIP(hipGetLastError());
    return MDC_OK;
}

int ddc_shape_check(const char* who, int64_t pairs, int ntaps, int decimate) {
    if (decimate < 1 || decimate > kMaxDecimate) { set_error("%s: decimate must be in 1..%d (got %d)", who, kMaxDecimate, decimate); return MDC_EINVAL; }
    if (ntaps < 1 || ntaps > kMaxTaps) { set_error("%s: ntaps must be in 1..%d (got %d)", who, kMaxTaps, ntaps); return MDC_EINVAL; }
    if (pairs < 0) { set_error("%s: negative pair count", who); return MDC_EINVAL; }
    return MDC_OK;
}

}  // namespace

}  // namespace mdc

using namespace mdc;

int64_t mdc_iq_ddc_out_count(int64_t pairs_in, int ntaps, int decimate) {
    const int rc = ddc_shape_check("mdc_iq_ddc_out_count", pairs_in, ntaps, decimate);
    return rc != MDC_OK ? (int64_t)rc : iq_span_count(pairs_in, ntaps, decimate);
}

int mdc_iq_ddc_nco_table(int16_t* cos_sin_host) {
    if (!cos_sin_host) { set_error("mdc_iq_ddc_nco_table: null buffer"); return MDC_EINVAL; }
    for (int k = 0; k < kNcoEntries; ++k) {
        cos_sin_host[2 * k] = (int16_t)(h_nco[k] & 0xFFFFu);
        cos_sin_host[2 * k + 1] = (int16_t)(h_nco[k] >> 16);
    }
    return MDC_OK;
}

int mdc_iq_ddc(const void* iq_dev, int format, int64_t pairs_in, uint32_t phase0, uint32_t phase_step, int decimate, const int16_t* taps_host,
               int ntaps, int16_t* out_dev, int64_t n_out, void* hip_stream) {
    int rc = iq_format_known("mdc_iq_ddc", format);
    if (rc != MDC_OK) return rc;
    if ((rc = ddc_shape_check("mdc_iq_ddc", pairs_in, ntaps, decimate)) != MDC_OK) return rc;
    if (!taps_host) { set_error("mdc_iq_ddc: null taps"); return MDC_EINVAL; }
    long abs_sum = 0;
    for (int k = 0; k < ntaps; ++k) abs_sum += taps_host[k] < 0 ? -(long)taps_host[k] : (long)taps_host[k];
    if (abs_sum > 65535) {
        set_error("mdc_iq_ddc: the taps' absolute values sum to %ld; at most 65535 keeps the 32-bit accumulation exact", abs_sum);
        return MDC_EINVAL;
    }
    if (n_out != iq_span_count(pairs_in, ntaps, decimate)) {
        set_error("mdc_iq_ddc: n_out is %lld, mdc_iq_ddc_out_count gives %lld", (long long)n_out, (long long)iq_span_count(pairs_in, ntaps, decimate));
        return MDC_EINVAL;
    }
    if ((rc = iq_pair_aligned("mdc_iq_ddc", "input", format, iq_dev)) != MDC_OK) return rc;
    if ((rc = iq_aligned("mdc_iq_ddc", "output", out_dev, 4)) != MDC_OK) return rc;
    if (n_out == 0) return MDC_OK;
    if (!iq_dev || !out_dev) { set_error("mdc_iq_ddc: null buffer"); return MDC_EINVAL; }
    DdcTaps taps{};
    for (int k = 0; k < ntaps; ++k) taps.pk[k >> 1] |= (unsigned)(uint16_t)taps_host[k] << (16 * (k & 1));
    const int ngroups = ((ntaps + 1) / 2 + kTapGroup - 1) / kTapGroup;
    const int tile_out = (kDdcTilePairs - ntaps) / decimate + 1;
    const unsigned char* p = static_cast<const unsigned char*>(iq_dev);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return guarded("mdc_iq_ddc", [&]() -> int {
        return with_format(format, [&](auto fmt) {
            return ddc_launch<decltype(fmt)::value>(p, pairs_in, phase0, phase_step, decimate, ngroups, tile_out, n_out, out_dev, taps, s); });
    });
}
