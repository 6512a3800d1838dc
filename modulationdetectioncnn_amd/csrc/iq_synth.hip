// mdc_iq_synth_plan / mdc_iq_synth_frames -- labelled I/Q frames of a balanced (modulation x SNR) grid, generated on the device
// (include/mdc.h, "frame synthesis"; exact integers; the numpy restatement is tests/iq_synth_ref.py).  One generic kernel: what a
// class is (alphabet or Gaussian source, pulse, LINEAR or PHASE, constants) is data in the plan blob, not code.
//
//   shape     one wave per frame, kSynWaves = 4 frames per work-group, two adjacent output pairs per lane (one 8-byte store per
//             lane, 512 contiguous bytes per wave).  Work-groups stride over the groups of four frames, at most kSynGridCap of
//             them (_cabi.SYNTH_GRID_CAP, SYNTH_GROUP_FRAMES).  The waves of a work-group hold different classes (adjacent frames
//             are adjacent cells), so each wave keeps its own symbols and its own class's tap image.
//   LDS       the oscillator table (4096 dwords, once per work-group) | per wave: the frame's symbols as two int32 planes
//             (2 x 144: a Gaussian symbol has 19 bits) and the class's branch-major taps (128 dwords, re | im << 16): 22.5 KiB.
//             Two work-group barriers per frame: every wave reaches both, with or without a frame (the walk is uniform).
//   draws     fmix32 (mdc_fmix32.h): per lane 16 for the noise of its four components, up to 3 symbols (x 4 for a Gaussian
//             source); the four frame-wide draws (timing, carrier phase and step, PHASE start) are computed by every lane.
//   filter    int32: the plan's branch bound (mdc.h) keeps every product and every partial sum of the definition's int64 sums
//             below 2^31, so 32-bit accumulation gives the same integers.
//   PHASE     the inclusive prefix sum of the 128 wrapping 32-bit increments: each lane sums its two, six shuffle steps scan the
//             64 lane sums (addition mod 2^32 is associative: any bracketing gives the same bits), the lane adds its own back.
//   channel   iq_mix.h's mixer arithmetic; the gains and the rounding shift in int64 (v_mad_i64_i32).
//   count     clamped components per lane in a register over all of the lane's frames, then shuffles, LDS, and ONE 64-bit
//             global atomic per work-group that has something to add.
// mdc_iq_synth_frames_faded is the kernel's second instantiation (include/mdc.h, "frame synthesis through a frequency-selective
// Rician channel"; tests/iq_synth_fading_ref.py), the same shape and walk:
//   head      the chain above runs for 128 + H samples, H = taps - 1 <= 15: the lanes below H take a third sample, n' = 128 + lane
//             (up to 160 symbols per plane; PHASE: a second four-step scan over those lanes on top of the first scan's total).
//   LDS       the mixed samples go through the wave's slice (2 x 144 int32), so a lane reads the T it needs: 27.5 KiB, five
//             work-groups per CU.  A third work-group barrier stands between writing and reading them; waves without a frame
//             meet it where they leave the iteration.
//   paths     delay lines in int32 (the record's bound), taps and path count wave-uniform from the kernel arguments; lane l draws
//             gain component l & 1 of path (l >> 1) & 3 and the wave reads the eight back; the sum over paths in int64.
//             79 VGPRs, no scratch; the first instantiation is unchanged (59 VGPRs, 22.5 KiB).
// The call only enqueues; vector memory for every store and atomic; no work-group waits on another.
// The plan blob's records, the draws and the run calls' plan check live in iq_synth_common.h, which mdc_iq_synth_capture
// (iq_synth_capture.hip) includes as well.
#include "iq_synth_common.h"

namespace mdc {

namespace {

constexpr int kSynThreads = 256;
constexpr int kSynWaves = kSynThreads / 64;      // frames per work-group and stride step (_cabi.SYNTH_GROUP_FRAMES)
constexpr long kSynGridCap = 2048;               // work-groups; beyond it they stride (_cabi.SYNTH_GRID_CAP)
constexpr int kSynMaxSymbols = 144;              // (127 + sps - 1) / sps + span <= 127 + 16 at sps = 1
constexpr int64_t kSynMaxFrames = (int64_t)1 << 30;
// mdc_iq_synth_frames_faded
constexpr int kSynMaxPaths = 4, kSynMaxDelayTaps = 16;
constexpr int kSynMaxSymbolsFaded = 160;         // (127 + 15 + sps - 1) / sps + span <= 142 + 16 at sps = 1
constexpr int kSynMaxHead = 144;                 // 128 + (16 - 1) mixed samples
constexpr unsigned kSynDrawPaths = 768;          // above the last symbol's counter (16 + 4 * 158 + 3), below the noise's
constexpr uint32_t kSynMaxDopplerStep = 1u << 30;

struct SynArgs {
    const SynClass* classes;
    const unsigned* points;
    const unsigned* taps;
    const int* gsig;
    const int* gnoise;
    u64 first_frame;
    long n;
    unsigned kseed, max_step, cell0;      // cell0 = first_frame mod (C S)
    int C, S, q;
};

// the fading record as the kernel reads it (uniform loads from the arguments): taps widened, fields side by side
struct SynFade {
    int d[kSynMaxPaths][kSynMaxDelayTaps];
    int los_re[kSynMaxPaths], los_im[kSynMaxPaths], scatter[kSynMaxPaths];
    int P, T;
    unsigned max_dop;
};
static_assert(sizeof(mdc_iq_synth_path) == 48 && sizeof(mdc_iq_synth_fading) == 208, "the fading record");
template <bool FADED> struct SynKernelArgs : SynArgs {};
template <> struct SynKernelArgs<true> : SynArgs { SynFade fd; };

// FADED: mdc_iq_synth_frames_faded -- the same chain over 128 + H samples (lanes below H take a third, n' = 128 + lane), the mixed
// samples through the wave's LDS slice, then the paths.  Everything the channel adds sits under `if constexpr (FADED)`: the other
// instantiation is mdc_iq_synth_frames' kernel as it was.
template <bool FADED>
__global__ __launch_bounds__(kSynThreads) void iq_synth_kernel(const SynKernelArgs<FADED> a, unsigned* __restrict__ out, int* __restrict__ labels,
                                                               int* __restrict__ snr_index, u64* __restrict__ saturated) {
    constexpr int kSymbols = FADED ? kSynMaxSymbolsFaded : kSynMaxSymbols;
    constexpr int E = FADED ? 3 : 2;      // samples of the unfaded chain per lane
    __shared__ unsigned nco[kNcoEntries];
    __shared__ int sym_re[kSynWaves][kSymbols], sym_im[kSynWaves][kSymbols];
    __shared__ int mix_re[kSynWaves][FADED ? kSynMaxHead : 1], mix_im[kSynWaves][FADED ? kSynMaxHead : 1];      // (FADED only)
    __shared__ unsigned tl[kSynWaves][kSynMaxTaps];
    __shared__ unsigned part[kSynWaves];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < kNcoEntries; i += kSynThreads) nco[i] = d_nco[i];
    int* sre = sym_re[wave];
    int* sim = sym_im[wave];
    unsigned* tw = tl[wave];
    const unsigned CS = (unsigned)(a.C * a.S);
    const long groups = (a.n + kSynWaves - 1) / kSynWaves;
    unsigned nsat = 0;
    int H = 0;      // head samples: taps - 1
    if constexpr (FADED) H = a.fd.T - 1;

    for (long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long i = g * kSynWaves + wave;      // < 2^30
        const bool active = i < a.n;              // uniform over the wave
        SynClass rec{};
        unsigned key = 0;
        int cls = 0, si = 0;
        __syncthreads();      // the table is in place; the previous frame's filter has read its symbols and taps
        if (active) {
            const unsigned cell = (a.cell0 + (unsigned)i) % CS;
            cls = (int)(cell % (unsigned)a.C);
            si = (int)(cell / (unsigned)a.C);
            key = syn_frame_key(a.kseed, a.first_frame + (u64)i);
            rec = a.classes[cls];
            int nsym = min(rec.nsym, kSynMaxSymbols);
            if constexpr (FADED) nsym = min((kSamples - 1 + H + rec.sps - 1) / rec.sps + rec.span, kSymbols);
            const int ntaps = min(rec.sps * rec.span, kSynMaxTaps);
            for (int k = lane; k < nsym; k += 64) {
                const unsigned j = kSynDrawSymbols + 4u * (unsigned)k;
                int re, im = 0;
                if (rec.source == MDC_SYNTH_GAUSS) {      // uniform over the wave
                    re = syn_gauss(key, j);
                } else {
                    const unsigned idx = (unsigned)(((u64)syn_draw(key, j) * (unsigned)rec.points) >> 32);
                    const unsigned pt = a.points[rec.point0 + (int)idx];
                    re = (int)(short)(pt & 0xFFFFu);
                    im = (int)(short)(pt >> 16);
                }
                sre[k] = re;
                sim[k] = im;
            }
            for (int t = lane; t < ntaps; t += 64) tw[t] = a.taps[rec.tap0 + t];
        }
        __syncthreads();
        if (!active) {      // (the barriers are above: every wave has passed both)
            if constexpr (FADED) __syncthreads();      // ... and the third, between the mixed samples and the paths, is met here
            continue;
        }

        const unsigned tau = (unsigned)(((u64)syn_draw(key, 0) * (unsigned)rec.sps) >> 32);
        const unsigned phi0 = syn_draw(key, 1);
        const unsigned step = (unsigned)(((u64)syn_draw(key, 2) * (2ull * a.max_step + 1ull)) >> 32) - a.max_step;
        int yr[E], yi[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            if (e == 2 && lane >= H) {      // (FADED only) no third sample: nothing is read, the increment below is 0
                yr[e] = yi[e] = 0;
                continue;
            }
            const unsigned p = (e < 2 ? 2u * (unsigned)lane + (unsigned)e : (unsigned)kSamples + (unsigned)lane) + tau;
            const unsigned m = p / (unsigned)rec.sps, b = p - m * (unsigned)rec.sps;
            const unsigned* tp = tw + b * (unsigned)rec.span;
            const int sb = (int)m + rec.span - 1;
            int ar = 0, ai = 0;
            for (int t = 0; t < rec.span; ++t) {
                const unsigned h = tp[t];
                const int hr = (int)(short)(h & 0xFFFFu), hi = (int)(short)(h >> 16);
                const int xr = sre[sb - t], xi = sim[sb - t];
                ar += xr * hr - xi * hi;
                ai += xr * hi + xi * hr;
            }
            yr[e] = (ar + 16384) >> 15;
            yi[e] = (ai + 16384) >> 15;
        }
        int zr[E], zi[E];
        if (rec.mode == MDC_SYNTH_PHASE) {      // uniform over the wave
            const unsigned inc0 = (unsigned)yr[0] * (unsigned)rec.factor, inc1 = (unsigned)yr[1] * (unsigned)rec.factor;
            const unsigned own = inc0 + inc1;
            unsigned x = own;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned t = __shfl_up(x, d, 64);
                if (lane >= d) x += t;
            }
            unsigned theta = syn_draw(key, 3) + (x - own);
            unsigned theta2 = 0;
            if constexpr (FADED) {      // the H increments behind the 128: a second scan over the lanes below 16, on top of the first's total
                unsigned x2 = (unsigned)yr[2] * (unsigned)rec.factor;
#pragma unroll
                for (int d = 1; d < kSynMaxDelayTaps; d <<= 1) {
                    const unsigned t = __shfl_up(x2, d, 64);
                    if (lane >= d) x2 += t;
                }
                theta2 = syn_draw(key, 3) + __shfl(x, 63, 64) + x2;
            }
#pragma unroll
            for (int e = 0; e < E; ++e) {
                theta = e == 2 ? theta2 : theta + (e == 0 ? inc0 : inc1);
                const unsigned cs = nco[theta >> 20];
                const int c = (int)(short)(cs & 0xFFFFu), s = (int)(short)(cs >> 16);
                zr[e] = ((c * rec.amp + 16384) >> 15) + rec.add_re;
                zi[e] = ((s * rec.amp + 16384) >> 15) + rec.add_im;
            }
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                zr[e] = yr[e] + rec.add_re;
                zi[e] = yi[e] + rec.add_im;
            }
        }
        const long gs = a.gsig[cls * a.S + si], gn = a.gnoise[si];
        const long half = 1l << (a.q - 1);
        int fr[2] = {0, 0}, fi[2] = {0, 0};      // (FADED only) y, which takes m's place below
        if constexpr (FADED) {
            int* mre = mix_re[wave];
            int* mim = mix_im[wave];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const unsigned n = e < 2 ? 2u * (unsigned)lane + (unsigned)e : (unsigned)kSamples + (unsigned)lane;
                const unsigned cs = nco[(phi0 + n * step) >> 20];
                const int c = (int)(short)(cs & 0xFFFFu), s = (int)(short)(cs >> 16);
                if (e < 2 || lane < H) {
                    mre[n] = (zr[e] * c - zi[e] * s + 32768) >> 16;
                    mim[n] = (zr[e] * s + zi[e] * c + 32768) >> 16;
                }
            }
            __syncthreads();      // the wave's 128 + H mixed samples are in its slice (waves without a frame meet this barrier above)
            const int P = a.fd.P, T = a.fd.T;
            // delay lines: int32 is exact (sum |d| <= 32767, |m| <= 32768); taps and path count are uniform, the taps come from the arguments
            int ar[kSynMaxPaths][2] = {}, ai[kSynMaxPaths][2] = {};
            for (int k = 0; k < T; ++k) {
                const int at = 2 * lane + H - k;
                const int x0r = mre[at], x0i = mim[at], x1r = mre[at + 1], x1i = mim[at + 1];
#pragma unroll
                for (int p = 0; p < kSynMaxPaths; ++p)
                    if (p < P) {
                        const int d = a.fd.d[p][k];
                        ar[p][0] += d * x0r;
                        ai[p][0] += d * x0i;
                        ar[p][1] += d * x1r;
                        ai[p][1] += d * x1i;
                    }
            }
            // path gains: lane l draws component l & 1 of path (l >> 1) & 3 (four draws each, not thirty-two per lane), read back below
            const int pl = (lane >> 1) & 3, cl = lane & 1;
            int los = 0, sc = 0;
#pragma unroll
            for (int p = 0; p < kSynMaxPaths; ++p)
                if (pl == p) {
                    los = cl ? a.fd.los_im[p] : a.fd.los_re[p];
                    sc = a.fd.scatter[p];
                }
            const unsigned jp = kSynDrawPaths + 16u * (unsigned)pl;
            const int gv = los + (int)(((long)syn_gauss(key, jp + 4u * (unsigned)cl) * sc + (1l << 17)) >> 18);
            const int dv = (int)syn_draw(key, jp + 8u + (unsigned)cl);      // psi (component 0's lane), nu's draw (component 1's)
            const unsigned max_dop = a.fd.max_dop;
            long sr[2] = {0, 0}, si[2] = {0, 0};
#pragma unroll
            for (int p = 0; p < kSynMaxPaths; ++p)
                if (p < P) {
                    const int gr = __shfl(gv, 2 * p, 64), gi = __shfl(gv, 2 * p + 1, 64);
                    const unsigned psi = (unsigned)__shfl(dv, 2 * p, 64);
                    const unsigned nu = (unsigned)(((u64)(unsigned)__shfl(dv, 2 * p + 1, 64) * (2ull * max_dop + 1ull)) >> 32) - max_dop;
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        int rr = gr, ri = gi;
                        if (max_dop != 0) {      // uniform over the grid
                            const unsigned cs = nco[(psi + (2u * (unsigned)lane + (unsigned)e) * nu) >> 20];
                            const int c = (int)(short)(cs & 0xFFFFu), s = (int)(short)(cs >> 16);
                            rr = (gr * c - gi * s + 16384) >> 15;
                            ri = (gr * s + gi * c + 16384) >> 15;
                        }
                        const int ur = (ar[p][e] + 8192) >> 14, ui = (ai[p][e] + 8192) >> 14;
                        sr[e] += (long)rr * ur - (long)ri * ui;
                        si[e] += (long)rr * ui + (long)ri * ur;
                    }
                }
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                fr[e] = (int)((sr[e] + 4096) >> 13);
                fi[e] = (int)((si[e] + 4096) >> 13);
            }
        }
        unsigned o[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const unsigned n = 2u * (unsigned)lane + (unsigned)e;
            int mr, mi;
            if constexpr (FADED) {
                mr = fr[e];
                mi = fi[e];
            } else {
                const unsigned cs = nco[(phi0 + n * step) >> 20];
                const int c = (int)(short)(cs & 0xFFFFu), s = (int)(short)(cs >> 16);
                mr = (zr[e] * c - zi[e] * s + 32768) >> 16;
                mi = (zr[e] * s + zi[e] * c + 32768) >> 16;
            }
            const int wr = syn_gauss(key, kSynDrawNoise + 8u * n), wi = syn_gauss(key, kSynDrawNoise + 8u * n + 4u);
            const long vr = ((long)mr * gs + (long)wr * gn + half) >> a.q, vi = ((long)mi * gs + (long)wi * gn + half) >> a.q;
            const long cr = vr < -32768 ? -32768 : vr > 32767 ? 32767 : vr, ci = vi < -32768 ? -32768 : vi > 32767 ? 32767 : vi;
            nsat += (cr != vr ? 1u : 0u) + (ci != vi ? 1u : 0u);
            o[e] = ((unsigned)cr & 0xFFFFu) | ((unsigned)ci << 16);
        }
        const uint2 v = make_uint2(o[0], o[1]);
        __builtin_memcpy(out + i * kSamples + 2 * lane, &v, sizeof(v));
        if (lane == 0) {
            if (labels) labels[i] = cls;
            if (snr_index) snr_index[i] = si;
        }
    }
    if (saturated == nullptr) return;      // uniform over the grid
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) nsat += __shfl_xor(nsat, d, 64);
    if (lane == 0) part[wave] = nsat;
    __syncthreads();
    if (tid == 0) {
        u64 s = 0;
#pragma unroll
        for (int w = 0; w < kSynWaves; ++w) s += part[w];
        if (s != 0) atomicAdd(saturated, s);
    }
}

// what both planner entries check of the records' shapes; on success the blob's layout and every class's first dwords
struct SynLayout {
    SynHeader h{};
    std::vector<int32_t> point0, tap0;
};

int synth_layout(const char* who, int32_t C, int32_t S, const mdc_iq_synth_class* cl, SynLayout& lay) {
    if (C < 1 || C > kSynMaxClasses) { set_error("%s: nclasses must be in 1..%d (got %d)", who, kSynMaxClasses, C); return MDC_EINVAL; }
    if (S < 1 || S > kSynMaxSnrs) { set_error("%s: nsnrs must be in 1..%d (got %d)", who, kSynMaxSnrs, S); return MDC_EINVAL; }
    if (!cl) { set_error("%s: null classes", who); return MDC_EINVAL; }
    lay.point0.resize((size_t)C);
    lay.tap0.resize((size_t)C);
    int32_t points = 0, taps = 0;
    for (int32_t k = 0; k < C; ++k) {
        const mdc_iq_synth_class& c = cl[k];
        if (c.reserved != 0) { set_error("%s: class %d: reserved must be 0 (got %d)", who, k, (int)c.reserved); return MDC_EINVAL; }
        if (c.source != MDC_SYNTH_ALPHABET && c.source != MDC_SYNTH_GAUSS) { set_error("%s: class %d: unknown source %d", who, k, c.source); return MDC_EINVAL; }
        if (c.mode != MDC_SYNTH_LINEAR && c.mode != MDC_SYNTH_PHASE) { set_error("%s: class %d: unknown mode %d", who, k, c.mode); return MDC_EINVAL; }
        if (c.source == MDC_SYNTH_ALPHABET ? pow2_log2(c.points, 0, 6) < 0 : c.points != 0) {
            set_error("%s: class %d: points must be a power of two in 1..%d for an alphabet and 0 for a Gaussian source (got %d)", who, k,
                      kSynMaxPoints, c.points);
            return MDC_EINVAL;
        }
        if (c.sps < 1 || c.sps > kSynMaxSps) { set_error("%s: class %d: sps must be in 1..%d (got %d)", who, k, kSynMaxSps, c.sps); return MDC_EINVAL; }
        if (c.span < 1 || c.span > kSynMaxSpan) { set_error("%s: class %d: span must be in 1..%d (got %d)", who, k, kSynMaxSpan, c.span); return MDC_EINVAL; }
        if (c.sps * c.span > kSynMaxTaps) {
            set_error("%s: class %d: sps * span must be at most %d taps (got %d * %d)", who, k, kSynMaxTaps, c.sps, c.span);
            return MDC_EINVAL;
        }
        if (c.first_point < 0 || c.first_tap < 0) { set_error("%s: class %d: negative first_point or first_tap", who, k); return MDC_EINVAL; }
        lay.point0[(size_t)k] = points;
        lay.tap0[(size_t)k] = taps;
        points += c.points;
        taps += c.sps * c.span;
    }
    SynHeader& h = lay.h;
    h.magic = kSynMagic;
    h.version = kSynVersion;
    h.C = C;
    h.S = S;
    h.off_classes = (int64_t)sizeof(SynHeader);
    h.off_points = h.off_classes + (int64_t)C * (int64_t)sizeof(SynClass);
    h.off_taps = round16(h.off_points + 4 * (int64_t)points);
    h.off_gsig = round16(h.off_taps + 4 * (int64_t)taps);
    h.off_gnoise = round16(h.off_gsig + 4 * (int64_t)C * S);
    h.bytes = round16(h.off_gnoise + 4 * (int64_t)S);
    return MDC_OK;
}

int iabs(int v) { return v < 0 ? -v : v; }

}  // namespace

}  // namespace mdc

using namespace mdc;

int64_t mdc_iq_synth_plan_bytes(int32_t nclasses, int32_t nsnrs, const mdc_iq_synth_class* classes_host) {
    int64_t bytes = MDC_EINVAL;
    const int rc = guarded("mdc_iq_synth_plan_bytes", [&]() -> int {
        SynLayout lay;
        const int r = synth_layout("mdc_iq_synth_plan_bytes", nclasses, nsnrs, classes_host, lay);
        if (r == MDC_OK) bytes = lay.h.bytes;
        return r;
    });
    return rc != MDC_OK ? (int64_t)rc : bytes;
}

int mdc_iq_synth_plan(const mdc_iq_synth_class* classes_host, int32_t nclasses, const int16_t* points_host, int64_t npoints, const int16_t* taps_host,
                      int64_t ntaps, const int32_t* gain_sig_host, int64_t ngain_sig, const int32_t* gain_noise_host, int32_t nsnrs, uint32_t max_step,
                      int32_t q, void* plan_host, int64_t plan_bytes) {
    static const char who[] = "mdc_iq_synth_plan";
    return guarded(who, [&]() -> int {
        SynLayout lay;
        int r = synth_layout(who, nclasses, nsnrs, classes_host, lay);
        if (r != MDC_OK) return r;
        const int32_t C = nclasses, S = nsnrs;
        if (npoints < 0 || (npoints > 0 && !points_host)) { set_error("%s: null points", who); return MDC_EINVAL; }
        if (ntaps < 0 || (ntaps > 0 && !taps_host)) { set_error("%s: null taps", who); return MDC_EINVAL; }
        if (ngain_sig != (int64_t)C * S) {
            set_error("%s: the signal gain table holds %lld entries, %d classes x %d SNRs need %lld", who, (long long)ngain_sig, C, S, (long long)C * S);
            return MDC_EINVAL;
        }
        if (!gain_sig_host || !gain_noise_host) { set_error("%s: null gain table", who); return MDC_EINVAL; }
        if (max_step > kSynMaxStep) { set_error("%s: max_step must be at most 2^30 (got %u)", who, max_step); return MDC_EINVAL; }
        if (q < 1 || q > kSynMaxQ) { set_error("%s: q must be in 1..%d (got %d)", who, kSynMaxQ, q); return MDC_EINVAL; }
        for (int32_t k = 0; k < C; ++k) {
            const mdc_iq_synth_class& c = classes_host[k];
            const int nt = c.sps * c.span;
            if ((int64_t)c.first_point + c.points > npoints) {
                set_error("%s: class %d: points %d .. %lld lie outside the %lld points given", who, k, c.first_point,
                          (long long)c.first_point + c.points - 1, (long long)npoints);
                return MDC_EINVAL;
            }
            if ((int64_t)c.first_tap + nt > ntaps) {
                set_error("%s: class %d: taps %d .. %lld lie outside the %lld taps given", who, k, c.first_tap, (long long)c.first_tap + nt - 1,
                          (long long)ntaps);
                return MDC_EINVAL;
            }
            int64_t amax = kSynGaussMax;
            if (c.source == MDC_SYNTH_ALPHABET) {
                amax = 0;
                for (int i = 0; i < 2 * c.points; ++i) amax = std::max<int64_t>(amax, iabs(points_host[2 * (int64_t)c.first_point + i]));
            }
            const int add = std::max(iabs(c.add_re), iabs(c.add_im));
            for (int b = 0; b < c.sps; ++b) {
                int64_t sum = 0;
                for (int i = 0; i < c.span; ++i) {
                    const int16_t* h = taps_host + 2 * ((int64_t)c.first_tap + b + (int64_t)i * c.sps);
                    sum += iabs(h[0]) + iabs(h[1]);
                }
                const int64_t bound = (sum * amax + 16384) >> 15;
                if (bound + add > 32767) {
                    set_error("%s: class %d: branch %d of the pulse (h[%d], h[%d + %d], ...) sums to %lld in absolute value, times the source's "
                              "largest component %lld that is %lld after the shift, plus the constant's %d: more than 32767", who, k, b, b, b, c.sps,
                              (long long)sum, (long long)amax, (long long)bound, add);
                    return MDC_EINVAL;
                }
            }
            if (c.mode == MDC_SYNTH_PHASE && iabs(c.amplitude) + add > 32767) {
                set_error("%s: class %d: |amplitude| + the constant's largest component must be at most 32767 (got %d + %d)", who, k,
                          iabs(c.amplitude), add);
                return MDC_EINVAL;
            }
        }
        SynHeader& h = lay.h;
        if (plan_bytes != h.bytes) {
            set_error("%s: plan_bytes is %lld, mdc_iq_synth_plan_bytes gives %lld", who, (long long)plan_bytes, (long long)h.bytes);
            return MDC_EINVAL;
        }
        if (!plan_host) { set_error("%s: null plan buffer", who); return MDC_EINVAL; }
        h.q = q;
        h.max_step = max_step;
        unsigned char* blob = static_cast<unsigned char*>(plan_host);
        memset(blob, 0, (size_t)h.bytes);
        memcpy(blob, &h, sizeof h);
        for (int32_t k = 0; k < C; ++k) {
            const mdc_iq_synth_class& c = classes_host[k];
            const SynClass e{c.source, c.points, c.sps, c.span, c.mode, c.phase_factor, c.amplitude, c.add_re, c.add_im,
                             lay.point0[(size_t)k], lay.tap0[(size_t)k], (kSamples - 1 + c.sps - 1) / c.sps + c.span};
            memcpy(blob + h.off_classes + (int64_t)k * (int64_t)sizeof e, &e, sizeof e);
            if (c.points) memcpy(blob + h.off_points + 4 * (int64_t)e.point0, points_host + 2 * (int64_t)c.first_point, 4 * (size_t)c.points);
            int16_t* img = reinterpret_cast<int16_t*>(blob + h.off_taps + 4 * (int64_t)e.tap0);
            for (int b = 0; b < c.sps; ++b)
                for (int i = 0; i < c.span; ++i)
                    memcpy(img + 2 * (b * c.span + i), taps_host + 2 * ((int64_t)c.first_tap + b + (int64_t)i * c.sps), 4);
        }
        memcpy(blob + h.off_gsig, gain_sig_host, 4 * (size_t)C * (size_t)S);
        memcpy(blob + h.off_gnoise, gain_noise_host, 4 * (size_t)S);
        return MDC_OK;
    });
}

// the fading record's preconditions (include/mdc.h); on success the record as the kernel reads it
static int synth_fading_check(const char* who, const mdc_iq_synth_fading* f, SynFade& fd) {
    if (!f) { set_error("%s: null fading record", who); return MDC_EINVAL; }
    if (f->paths < 1 || f->paths > kSynMaxPaths) { set_error("%s: fading: paths must be in 1..%d (got %d)", who, kSynMaxPaths, f->paths); return MDC_EINVAL; }
    if (f->taps < 1 || f->taps > kSynMaxDelayTaps) { set_error("%s: fading: taps must be in 1..%d (got %d)", who, kSynMaxDelayTaps, f->taps); return MDC_EINVAL; }
    if (f->max_doppler_step > kSynMaxDopplerStep) {
        set_error("%s: fading: max_doppler_step must be at most 2^30 (got %u)", who, f->max_doppler_step);
        return MDC_EINVAL;
    }
    if (f->reserved != 0) { set_error("%s: fading: reserved must be 0 (got %d)", who, f->reserved); return MDC_EINVAL; }
    fd = SynFade{};
    fd.P = f->paths;
    fd.T = f->taps;
    fd.max_dop = f->max_doppler_step;
    for (int p = 0; p < kSynMaxPaths; ++p) {
        const mdc_iq_synth_path& q = f->path[p];
        if (q.reserved[0] != 0 || q.reserved[1] != 0) { set_error("%s: fading: path %d: reserved must be 0", who, p); return MDC_EINVAL; }
        int64_t sum = 0;
        for (int k = 0; k < kSynMaxDelayTaps; ++k) {
            if (k >= f->taps && q.delay_taps[k] != 0) {
                set_error("%s: fading: path %d: delay_taps[%d] must be 0 with %d taps (got %d)", who, p, k, f->taps, (int)q.delay_taps[k]);
                return MDC_EINVAL;
            }
            sum += iabs(q.delay_taps[k]);
            fd.d[p][k] = q.delay_taps[k];
        }
        if (p >= f->paths) {
            if (sum != 0 || q.los_re != 0 || q.los_im != 0 || q.scatter != 0) {
                set_error("%s: fading: path %d: every field of a path beyond the %d in use must be 0", who, p, f->paths);
                return MDC_EINVAL;
            }
            continue;
        }
        if (sum > 32767) {
            set_error("%s: fading: path %d: the delay taps sum to %lld in absolute value: more than 32767", who, p, (long long)sum);
            return MDC_EINVAL;
        }
        if (q.scatter < 0) { set_error("%s: fading: path %d: scatter must be >= 0 (got %d)", who, p, q.scatter); return MDC_EINVAL; }
        const int64_t los = std::max(iabs(q.los_re), iabs(q.los_im));
        if (los + (int64_t)q.scatter > 32767) {
            set_error("%s: fading: path %d: max(|los_re|, |los_im|) + scatter must be at most 32767 (got %lld + %d)", who, p, (long long)los, q.scatter);
            return MDC_EINVAL;
        }
        fd.los_re[p] = q.los_re;
        fd.los_im[p] = q.los_im;
        fd.scatter[p] = q.scatter;
    }
    return MDC_OK;
}

// both entries: `fading` is null for mdc_iq_synth_frames
static int synth_frames(const char* who, const void* plan_host, const void* plan_dev, int64_t plan_bytes, uint64_t seed, uint64_t first_frame,
                        int64_t n_frames, int16_t* iq_out_dev, int32_t* labels_dev, int32_t* snr_index_dev, uint64_t* saturated_dev,
                        const SynFade* fading, void* hip_stream) {
    SynHeader h;
    int rc = syn_plan_open(who, plan_host, plan_bytes, h);
    if (rc != MDC_OK) return rc;
    if (n_frames < 0 || n_frames > kSynMaxFrames) { set_error("%s: n_frames must be in 0..2^30 (got %lld)", who, (long long)n_frames); return MDC_EINVAL; }
    if ((rc = iq_aligned(who, "output", iq_out_dev, 4)) != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "labels_dev", labels_dev, 4)) != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "snr_index_dev", snr_index_dev, 4)) != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "saturated_dev", saturated_dev, 8)) != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "plan_dev", plan_dev, 8)) != MDC_OK) return rc;
    if (n_frames == 0) return MDC_OK;
    if (!iq_out_dev || !plan_dev) { set_error("%s: null buffer", who); return MDC_EINVAL; }
    if ((rc = syn_plan_classes_check(who, plan_host, h)) != MDC_OK) return rc;
    const unsigned char* pd = static_cast<const unsigned char*>(plan_dev);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return guarded(who, [&]() -> int {
        SynArgs a{};
        a.classes = reinterpret_cast<const SynClass*>(pd + h.off_classes);
        a.points = reinterpret_cast<const unsigned*>(pd + h.off_points);
        a.taps = reinterpret_cast<const unsigned*>(pd + h.off_taps);
        a.gsig = reinterpret_cast<const int*>(pd + h.off_gsig);
        a.gnoise = reinterpret_cast<const int*>(pd + h.off_gnoise);
        a.first_frame = first_frame;
        a.n = (long)n_frames;
        a.kseed = syn_seed_key(seed);
        a.max_step = h.max_step;
        a.cell0 = (unsigned)(first_frame % (uint64_t)(h.C * h.S));
        a.C = h.C;
        a.S = h.S;
        a.q = h.q;
        const long groups = ((long)n_frames + kSynWaves - 1) / kSynWaves;
        const dim3 grid((unsigned)(groups < kSynGridCap ? groups : kSynGridCap));
        unsigned* out = reinterpret_cast<unsigned*>(iq_out_dev);
        u64* sat = reinterpret_cast<u64*>(saturated_dev);
        if (fading) {
            SynKernelArgs<true> af{};
            static_cast<SynArgs&>(af) = a;
            af.fd = *fading;
            hipLaunchKernelGGL(iq_synth_kernel<true>, grid, dim3(kSynThreads), 0, s, af, out, labels_dev, snr_index_dev, sat);
        } else {
            SynKernelArgs<false> au{};
            static_cast<SynArgs&>(au) = a;
            hipLaunchKernelGGL(iq_synth_kernel<false>, grid, dim3(kSynThreads), 0, s, au, out, labels_dev, snr_index_dev, sat);
        }
        MDC_HIP(hipGetLastError());
        return MDC_OK;
    });
}

int mdc_iq_synth_frames(const void* plan_host, const void* plan_dev, int64_t plan_bytes, uint64_t seed, uint64_t first_frame, int64_t n_frames,
                        int16_t* iq_out_dev, int32_t* labels_dev, int32_t* snr_index_dev, uint64_t* saturated_dev, void* hip_stream) {
    return synth_frames("mdc_iq_synth_frames", plan_host, plan_dev, plan_bytes, seed, first_frame, n_frames, iq_out_dev, labels_dev, snr_index_dev,
                        saturated_dev, nullptr, hip_stream);
}

int mdc_iq_synth_frames_faded(const void* plan_host, const void* plan_dev, int64_t plan_bytes, uint64_t seed, uint64_t first_frame, int64_t n_frames,
                              int16_t* iq_out_dev, int32_t* labels_dev, int32_t* snr_index_dev, uint64_t* saturated_dev,
                              const mdc_iq_synth_fading* fading_host, void* hip_stream) {
    static const char who[] = "mdc_iq_synth_frames_faded";
    SynFade fd;
    const int rc = synth_fading_check(who, fading_host, fd);
    if (rc != MDC_OK) return rc;
    return synth_frames(who, plan_host, plan_dev, plan_bytes, seed, first_frame, n_frames, iq_out_dev, labels_dev, snr_index_dev, saturated_dev, &fd,
                        hip_stream);
}
