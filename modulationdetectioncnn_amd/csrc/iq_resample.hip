// mdc_iq_resample -- tune, low-pass and resample a wideband integer I/Q capture by a rational factor L / D on the device, in
// exact integer arithmetic (include/mdc.h, "rational resampler"; the numpy int64 restatement is tests/iq_resample_ref.py).
// It is mdc_iq_ddc (iq_ddc.hip) with L - 1 zeros between the mixed samples, computed without the zeros: output j reads the
// mixed samples from s_j = ceil(j D / L) on through BRANCH r_j = s_j L - j D of the prototype, the taps h[r_j + i L].
//
//   tile      `tile_out` = q L outputs with q = (kIqTilePairs - B) / D, B = ceil(T / L) the longest branch: such a tile starts
//             at the input pair t q D EXACTLY (and at branch 0), so everything inside a tile is 32-bit arithmetic on local
//             indices, and it reads at most q D + B <= kIqTilePairs pairs.  Work-groups stride over the tiles (kResGridCap).
//   mix       the DDC's, written out here: quads of pairs -> two planar int16 LDS images, 33-dword stride.
//   taps      adjacent outputs use different branches, so the taps cannot be wave-uniform scalar operands as in the DDC.  The
//             host reorders them BRANCH-MAJOR into packed pairs (branch r, dword u: h[r + 2uL] | h[r + (2u+1)L] << 16, zeros
//             beyond T; every branch padded to whole groups of kResTapGroup dwords, the branch stride made ODD so that the L
//             branches of a wave's lanes start on L different banks); that image travels by value as a kernel argument
//             (<= kResTapDwords dwords: no copy to wait for, nothing to allocate) and each work-group copies it into LDS once.
//   filter    the DDC's, written out here with groups of kResTapGroup dwords: one lane per output from the local sample s on
//             against its branch's pairs -- two sample dwords (re, im) and one tap dword from LDS per two dot products.  ODD
//             instantiations: any class of outputs starts on an odd local sample.  An empty branch (r >= T) is all padding:
//             its outputs are (0 + 8192) >> 14 = 0.
// Everything the filter reads beyond the tile's last needed sample (the branches' zero padding times it) is still written by
// the mix step -- zeros beyond the capture -- so the result never depends on stale LDS.  |acc| <= 32767 * 65535 per branch.
// The call only enqueues; vector memory for every store.
// iq_mix.h describes both stages and holds them as mix_tile and fir_output, which the DDC calls.  This kernel keeps its own
// copies, line for line the same: with either call in its place rows of tools/resample_probe.py measured up to 6 % slower on the
// MI355X, outside the spread of this code against itself (the rows: DESIGN.md 5.16, profiles/iq_frontend_ab.txt).  A change to
// either stage is made in both places; tests/test_iq_resample_gpu.py::test_one_branch_is_the_ddc holds them to the same bits.
#include "iq_resample_plan.h"      // limits, tiling and the tap image, shared with mdc_iq_extract

namespace mdc {

namespace {

template <int FMT, bool ODD>
__global__ __launch_bounds__(kResThreads) void iq_resample_kernel(const unsigned char* __restrict__ iq, long pairs, unsigned phase0, unsigned step,
                                                                  const ResPlan plan, long n_out, long ntiles, unsigned* __restrict__ out,
                                                                  const ResTaps taps) {
    __shared__ unsigned lds[kNcoEntries + kResTapDwords + 2 * kPlaneDwords];
    unsigned* nco = lds;
    unsigned* tl = lds + kNcoEntries;
    unsigned* re = tl + kResTapDwords;
    unsigned* im = re + kPlaneDwords;
    const int tid = threadIdx.x;
    const unsigned L = (unsigned)plan.L, D = (unsigned)plan.D;
    const int ngroups = plan.ngroups;
    for (int i = tid; i < kNcoEntries; i += kResThreads) nco[i] = d_nco[i];
    for (int i = tid; i < plan.tapdw; i += kResThreads) tl[i] = taps.pk[i];

    for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long out0 = t * plan.tile_out, in0 = t * plan.tile_in;
        const long left = n_out - out0;
        const int nout = left < plan.tile_out ? (int)left : plan.tile_out;
        // local pairs the filter reads: the last output's start, its branch's tap groups, one more dword for the ODD look-ahead
        const int last = (int)(((unsigned)(nout - 1) * D + L - 1) / L);
        const int span = last + 2 * kResTapGroup * ngroups + 2;      // <= kIqTilePairs + 9
        const int quads = (span + 3) >> 2;
        __syncthreads();      // table and taps are in place; the previous tile's filter has read its samples
        for (int q = tid; q < quads; q += kResThreads) {
            const long n = in0 + 4 * (long)q;
            int I[4], Q[4], mr[4], mi[4];
            load_quad<FMT>(iq, n, pairs, I, Q);
            const unsigned phi = phase0 + (unsigned)(unsigned long)n * step;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned cs = nco[(phi + (unsigned)e * step) >> 20];
                const int c = (int)(short)(cs & 0xFFFFu), s = (int)(short)(cs >> 16);
                mr[e] = (I[e] * c - Q[e] * s + 32768) >> 16;
                mi[e] = (I[e] * s + Q[e] * c + 32768) >> 16;
            }
            const int a = lds_slot(2 * q), b = lds_slot(2 * q + 1);
            re[a] = ((unsigned)mr[0] & 0xFFFFu) | ((unsigned)mr[1] << 16);
            re[b] = ((unsigned)mr[2] & 0xFFFFu) | ((unsigned)mr[3] << 16);
            im[a] = ((unsigned)mi[0] & 0xFFFFu) | ((unsigned)mi[1] << 16);
            im[b] = ((unsigned)mi[2] & 0xFFFFu) | ((unsigned)mi[3] << 16);
        }
        __syncthreads();
        for (int j = tid; j < nout; j += kResThreads) {
            const unsigned jd = (unsigned)j * D;                     // < tile_in * L <= 2^18
            const unsigned start = (jd + L - 1) / L, branch = start * L - jd;
            const int base = (int)(start >> 1);
            const unsigned sh = (start & 1u) << 4;
            const unsigned* tp = tl + branch * (unsigned)plan.stride;
            int ar = 0, ai = 0;
            unsigned cr = 0, ci = 0;
            if (ODD) { cr = re[lds_slot(base)]; ci = im[lds_slot(base)]; }
            for (int g = 0; g < ngroups; ++g) {
#pragma unroll
                for (int u = 0; u < kResTapGroup; ++u) {
                    const unsigned tap = tp[kResTapGroup * g + u];
                    unsigned wr, wi;
                    if (ODD) {
                        const int idx = lds_slot(base + kResTapGroup * g + u + 1);
                        const unsigned nr = re[idx], ni = im[idx];
                        wr = __builtin_amdgcn_alignbit(nr, cr, sh);
                        wi = __builtin_amdgcn_alignbit(ni, ci, sh);
                        cr = nr;
                        ci = ni;
                    } else {
                        const int idx = lds_slot(base + kResTapGroup * g + u);
                        wr = re[idx];
                        wi = im[idx];
                    }
                    ar = dot2(wr, tap, ar);
                    ai = dot2(wi, tap, ai);
                }
            }
            const int r = sat16((ar + 8192) >> 14), i = sat16((ai + 8192) >> 14);
            out[out0 + j] = ((unsigned)r & 0xFFFFu) | ((unsigned)i << 16);
        }
    }
}

template <int FMT>
int resample_launch(const unsigned char* iq, int64_t pairs, uint32_t phase0, uint32_t step, const ResPlan& plan, int64_t n_out, int16_t* out,
                    const ResTaps& taps, hipStream_t s) {
    const long ntiles = (n_out + plan.tile_out - 1) / plan.tile_out;
    const dim3 g((unsigned)(ntiles < kResGridCap ? ntiles : kResGridCap)), b(kResThreads);
    unsigned* o = reinterpret_cast<unsigned*>(out);
    if (plan.odd) hipLaunchKernelGGL((iq_resample_kernel<FMT, true>), g, b, 0, s, iq, (long)pairs, phase0, step, plan, (long)n_out, ntiles, o, taps);
    else          hipLaunchKernelGGL((iq_resample_kernel<FMT, false>), g, b, 0, s, iq, (long)pairs, phase0, step, plan, (long)n_out, ntiles, o, taps);
    MDC_HIP(hipGetLastError());
    return MDC_OK;
}

}  // namespace

}  // namespace mdc

using namespace mdc;

int64_t mdc_iq_resample_out_count(int64_t pairs_in, int ntaps, int interpolate, int decimate) {
    const int rc = resample_shape_check("mdc_iq_resample_out_count", pairs_in, ntaps, interpolate, decimate);
    return rc != MDC_OK ? (int64_t)rc : resample_out_count(pairs_in, ntaps, interpolate, decimate);
}

int mdc_iq_resample(const void* iq_dev, int format, int64_t pairs_in, uint32_t phase0, uint32_t phase_step, int interpolate, int decimate,
                    const int16_t* taps_host, int ntaps, int16_t* out_dev, int64_t n_out, void* hip_stream) {
    int rc = iq_format_known("mdc_iq_resample", format);
    if (rc != MDC_OK) return rc;
    if ((rc = resample_shape_check("mdc_iq_resample", pairs_in, ntaps, interpolate, decimate)) != MDC_OK) return rc;
    if (!taps_host) { set_error("mdc_iq_resample: null taps"); return MDC_EINVAL; }
    for (int r = 0; r < interpolate && r < ntaps; ++r) {
        long abs_sum = 0;
        for (int k = r; k < ntaps; k += interpolate) abs_sum += taps_host[k] < 0 ? -(long)taps_host[k] : (long)taps_host[k];
        if (abs_sum > 65535) {
            set_error("mdc_iq_resample: the absolute values of branch %d of the taps (h[%d], h[%d + %d], ...) sum to %ld; at most 65535 keeps the "
                      "32-bit accumulation exact", r, r, r, interpolate, abs_sum);
            return MDC_EINVAL;
        }
    }
    const int64_t want = resample_out_count(pairs_in, ntaps, interpolate, decimate);
    if (n_out != want) {
        set_error("mdc_iq_resample: n_out is %lld, mdc_iq_resample_out_count gives %lld", (long long)n_out, (long long)want);
        return MDC_EINVAL;
    }
    if ((rc = iq_pair_aligned("mdc_iq_resample", "input", format, iq_dev)) != MDC_OK) return rc;
    if ((rc = iq_aligned("mdc_iq_resample", "output", out_dev, 4)) != MDC_OK) return rc;
    if (n_out == 0) return MDC_OK;
    if (!iq_dev || !out_dev) { set_error("mdc_iq_resample: null buffer"); return MDC_EINVAL; }
    ResTaps taps{};
    ResPlan plan{};
    if (!resample_plan(interpolate, decimate, taps_host, ntaps, plan, taps.pk)) {
        set_error("mdc_iq_resample: internal: the branch-major tap image of %d taps in %d branches exceeds %d dwords", ntaps, interpolate, kResTapDwords);
        return MDC_EINVAL;
    }
    const unsigned char* p = static_cast<const unsigned char*>(iq_dev);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return guarded("mdc_iq_resample", [&]() -> int {
        return with_format(format, [&](auto fmt) { return resample_launch<decltype(fmt)::value>(p, pairs_in, phase0, phase_step, plan, n_out, out_dev, taps, s); });
    });
}
