// mdc_iq_synth_scene / mdc_iq_synth_capture -- a scene of up to 32 emitters rendered into ONE wideband ci16 capture on the device
// (include/mdc.h, "capture synthesis"; exact integers; the numpy restatement is tests/iq_synth_capture_ref.py).  The inverse of
// mdc_iq_extract: each emitter is a class of a plan of mdc_iq_synth_plan (its source, pulse and mode lines are the frames', at the
// class's samples per symbol, over an unbounded symbol stream), gated by a burst schedule, interpolated by L / D to the capture's
// rate, mixed to its (possibly hopping) carrier, and summed with the others and the noise in int64.
//
//   shape     one work-group of 256 threads per tile of kCapTile = 1024 capture pairs, four adjacent pairs per lane, one 16-byte
//             store per lane (the capture's last, partial tile pair by pair with bounds).  At most kCapGridCap work-groups; beyond
//             it they stride over the tiles.
//   emitters  per tile, lane e of the first wave decides whether emitter e's gate is on anywhere in the tile's baseband range (all
//             emitters side by side), a ballot makes the decisions one mask in LDS, and the work-group loops over its set bits: an
//             emitter that is off over the whole tile costs nothing more (its mixed samples are exactly 0).  The mask is uniform,
//             so every barrier inside the loop is met by the whole work-group.
//   per (emitter, tile): the tile's first output needs baseband samples from b0 = m(n0) - (K - 1) on, K = ceil(T / L); its last
//             m(n0 + 1023): at most 1023 D / L + 1 + K <= 1088 samples.  (1) the symbols those reach (<= 1104, two int32 planes: a
//             Gaussian symbol has 19 bits), the class's pulse (branch-major dwords) and the emitter's interpolation taps
//             (zero-padded to K L) go to LDS; (2) each thread runs the pulse for five adjacent baseband samples, PHASE: a
//             work-group scan of the 32-bit increments on top of the tile's start phase; the gate; z packed (re | im << 16) to
//             LDS; (3) each lane applies its outputs' branch taps from LDS (int32: the branch bound), clamps, mixes with the
//             carrier (d_nco in LDS) and adds m * gain into its int64 accumulators (v_mad_i64_i32).
//   divisions 64-bit divisions only on uniform values, once per (emitter, tile): the tile's first P = n0 D + T - 1 by L and the
//             gate's first baseband sample by the period.  Per sample, 32-bit arithmetic on the distance from those.
//   PHASE     theta at b0 is theta0 plus all increments before b0, gated stretches included.  Scenes with a PHASE emitter run two
//             launches ahead of the main one: cap_phase_sums adds up the increments of [b0(t), b0(t + 1)) per (PHASE emitter,
//             tile t) into the workspace, cap_phase_scan (one work-group per PHASE emitter) turns them into exclusive prefix sums.
//             Addition mod 2^32 is associative: any bracketing gives the same bits.  A scene without one is ONE launch.
//   count     clamped components (interpolation and output clamps alike) per lane in a register, then shuffles, LDS and one
//             64-bit global atomic per work-group that has something to add.
// The call only enqueues; vector memory for every store and atomic; no work-group waits on another.
#include "iq_synth_common.h"

#include <vector>

namespace mdc {

namespace {

constexpr uint32_t kScnMagic = 0x4353434Du;      // "MCSC"
constexpr uint32_t kScnVersion = 1;
constexpr int kCapThreads = 256;
constexpr int kCapWaves = kCapThreads / 64;
constexpr int kCapTile = 1024;                   // capture pairs per tile (_cabi.SYNTH_CAPTURE_TILE)
constexpr int kCapPerLane = kCapTile / kCapThreads;
constexpr long kCapGridCap = 4096;               // work-groups; beyond it they stride (_cabi.SYNTH_CAPTURE_GRID_CAP)
constexpr int kScnMaxEmitters = 32, kScnMaxL = 32, kScnMaxTaps = 1024, kScnMaxBranch = 64, kScnMaxHops = 8;
constexpr int64_t kScnMaxBranchAbsSum = 65535;
constexpr int64_t kScnMaxTime = (int64_t)1 << 52;       // start, on, period
constexpr int64_t kCapMaxPairs = (int64_t)1 << 34;
constexpr int kCapMaxBase = kCapTile + kScnMaxBranch;                 // 1088 baseband samples per (emitter, tile)
constexpr int kCapBasePerThread = (kCapMaxBase + kCapThreads - 1) / kCapThreads;      // 5
constexpr int kCapMaxSymbols = kCapMaxBase + kSynMaxSpan;            // 1104
constexpr int kCapTapSlots = kScnMaxTaps + kScnMaxL;                  // taps zero-padded to K L < T + L

// the scene blob: ScnHeader | E ScnEmitter | taps (int16); every part starts on a multiple of 16 bytes
struct ScnHeader {
    uint32_t magic, version;
    int32_t E, q, gain_noise, dc_re, dc_im, nphase;
    int64_t ntaps, bytes, off_emitters, off_taps;
};
struct ScnEmitter {
    mdc_iq_synth_emitter e;
    int32_t K;                 // ceil(ntaps / interpolate)
    int32_t phase_slot;        // the emitter's row in the workspace: its rank among the PHASE emitters, or -1
};
static_assert(sizeof(mdc_iq_synth_emitter) == 96 && sizeof(ScnEmitter) == 104 && sizeof(ScnHeader) == 64, "the scene blob's records");

constexpr u64 kFieldSymbols = 0, kFieldConstants = 1, kFieldDwell = 2, kFieldNoise = 3;
__host__ __device__ __forceinline__ u64 cap_f(int e_plus_1, u64 field, u64 low) { return ((u64)e_plus_1 << 56) + (field << 52) + low; }
__host__ __device__ __forceinline__ unsigned cap_hop(unsigned kseed, int em, u64 w, int hops) {
    return (unsigned)(((u64)syn_draw(syn_frame_key(kseed, cap_f(em + 1, kFieldDwell, w)), 0) * (unsigned)hops) >> 32);
}

struct CapArgs {
    const ScnEmitter* emitters;
    const short* taps;
    const SynClass* classes;
    const unsigned* points;
    const unsigned* ptaps;      // the plan's tap images
    unsigned* prefix;           // workspace: nphase rows of `tiles` dwords
    long n, tiles;
    unsigned kseed;
    int E, q, gain_noise, dc_re, dc_im;
};

// an emitter's schedule relative to a baseband index `from`: everything later is 32-bit arithmetic on the distance from it
struct Gate {
    long start, on, period;
    long from;       // first baseband index the walk covers
    long x0;         // from - start (may be negative: not yet started)
    long ph0, w0;    // period > 0 and x0 >= 0: (x0 mod period, x0 / period); else 0
};
__device__ __forceinline__ Gate gate_at(const mdc_iq_synth_emitter& e, long from) {
    Gate g{e.start, e.on, e.period, from, from - e.start, 0, 0};
    if (g.period > 0 && g.x0 > 0) {      // uniform: one 64-bit division per (emitter, tile)
        g.w0 = g.x0 / g.period;
        g.ph0 = g.x0 - g.w0 * g.period;
    }
    return g;
}
// is the emitter on at from + j (0 <= j < 2^15)?  *dwell: w(from + j)
__device__ __forceinline__ bool gate_on(const Gate& g, int j, long* dwell) {
    long x = g.x0 + j;
    *dwell = 0;
    if (x < 0) return false;
    if (g.period == 0) return g.on == 0 || x < g.on;
    long ph, w;
    if (g.x0 >= 0) { ph = g.ph0 + j; w = g.w0; }
    else { ph = x; w = 0; }                              // started inside the walk: x < 2^15
    if (ph >= g.period) {
        if (g.period < 65536) {                          // ph < 2^16 + 2^15: a 32-bit division
            const unsigned qn = (unsigned)ph / (unsigned)g.period;
            ph -= (long)qn * g.period;
            w += qn;
        } else {                                         // ph < period + 2^15 < 2 period
            ph -= g.period;
            w += 1;
        }
    }
    *dwell = w;
    return ph < g.on;
}
// is the emitter on anywhere in from .. from + count - 1?  (uniform)
__device__ __forceinline__ bool gate_any(const Gate& g, int count) {
    const long last = g.x0 + count - 1;
    if (last < 0) return false;
    const long first = g.x0 > 0 ? g.x0 : 0;
    if (g.period == 0) return g.on == 0 || first < g.on;
    if (g.on == 0) return false;
    const long ph = g.x0 > 0 ? g.ph0 : 0;
    if (ph < g.on) return true;
    return first + (g.period - ph) <= last;
}

// LDS of one (emitter, range): the symbols and the class's pulse
struct BaseLds {
    int sym_re[kCapMaxSymbols + 8], sym_im[kCapMaxSymbols + 8];
    unsigned pulse[kSynMaxTaps];
};

// symbols k0 .. k0 + nsym - 1 of emitter em and the class's pulse into LDS (the caller puts a barrier behind it)
__device__ __forceinline__ void base_fill(BaseLds& L, const CapArgs& a, int em, const SynClass& rec, long k0, int nsym, int tid) {
    nsym = min(nsym, kCapMaxSymbols + 8);
    for (int s = tid; s < nsym; s += kCapThreads) {
        const u64 k = (u64)(k0 + s);
        const unsigned key = syn_frame_key(a.kseed, cap_f(em + 1, kFieldSymbols, k >> 7));
        const unsigned j = kSynDrawSymbols + 4u * (unsigned)(k & 127u);
        int re, im = 0;
        if (rec.source == MDC_SYNTH_GAUSS) {
            re = syn_gauss(key, j);
        } else {
            const unsigned idx = (unsigned)(((u64)syn_draw(key, j) * (unsigned)rec.points) >> 32);
            const unsigned pt = a.points[rec.point0 + (int)idx];
            re = (int)(short)(pt & 0xFFFFu);
            im = (int)(short)(pt >> 16);
        }
        L.sym_re[s] = re;
        L.sym_im[s] = im;
    }
    const int ntaps = min(rec.sps * rec.span, kSynMaxTaps);
    for (int t = tid; t < ntaps; t += kCapThreads) L.pulse[t] = a.ptaps[rec.tap0 + t];
}

// y of the baseband sample at stream position p = i + tau (the frames' pulse line), symbols from k0 on in LDS
__device__ __forceinline__ void base_y(const BaseLds& L, const SynClass& rec, long p, long k0, int* yr, int* yi) {
    // p / sps: p < 2^53, sps <= 16 -- by the distance from k0 sps, which is below 2^15
    const unsigned d = (unsigned)(p - k0 * rec.sps);
    const unsigned m = d / (unsigned)rec.sps, b = d - m * (unsigned)rec.sps;
    const unsigned* tp = L.pulse + b * (unsigned)rec.span;
    const int sb = (int)m + rec.span - 1;
    int ar = 0, ai = 0;
    for (int t = 0; t < rec.span; ++t) {
        const unsigned h = tp[t];
        const int hr = (int)(short)(h & 0xFFFFu), hi = (int)(short)(h >> 16);
        const int xr = L.sym_re[sb - t], xi = L.sym_im[sb - t];
        ar += xr * hr - xi * hi;
        ai += xr * hi + xi * hr;
    }
    *yr = (ar + 16384) >> 15;
    *yi = (ai + 16384) >> 15;
}

// first baseband sample tile t of an emitter reads: m(n0) - (K - 1) with m(n0) = (n0 D + T - 1) / L; *r0 = (n0 D + T - 1) mod L
__device__ __forceinline__ long tile_base(const ScnEmitter& s, long tile, int* r0) {
    const long P0 = tile * kCapTile * (long)s.e.decimate + s.e.ntaps - 1;
    const long m0 = P0 / s.e.interpolate;
    *r0 = (int)(P0 - m0 * s.e.interpolate);
    return m0 - (s.K - 1);
}

// the work-group's inclusive scan of one value per thread (mod 2^32); part: kCapWaves dwords of LDS.  Two barriers.
__device__ __forceinline__ unsigned block_scan(unsigned own, unsigned* part, int tid, unsigned* total) {
    const int lane = tid & 63, wave = tid >> 6;
    unsigned x = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(x, d, 64);
        if (lane >= d) x += t;
    }
    __syncthreads();      // part's previous readers are done
    if (lane == 63) part[wave] = x;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kCapWaves; ++w) {
        if (w < wave) before += part[w];
        all += part[w];
    }
    *total = all;
    return x + before;
}

// workspace[slot][tile] = sum of the PHASE increments of the emitter's baseband samples b0(tile) .. b0(tile + 1) - 1
__global__ __launch_bounds__(kCapThreads) void cap_phase_sums(const CapArgs a) {
    __shared__ BaseLds L;
    __shared__ unsigned part[kCapWaves];
    const int tid = threadIdx.x;
    for (int em = 0; em < a.E; ++em) {
        const ScnEmitter s = a.emitters[em];
        if (s.phase_slot < 0) continue;      // uniform
        const SynClass rec = a.classes[s.e.cls];
        const unsigned tau = (unsigned)(((u64)syn_draw(syn_frame_key(a.kseed, cap_f(em + 1, kFieldConstants, 0)), 0) * (unsigned)rec.sps) >> 32);
        for (long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
            int r0;
            const long b0 = tile_base(s, tile, &r0), b1 = tile_base(s, tile + 1, &r0);
            const int nb = min((int)(b1 - b0), kCapMaxBase);      // <= 1024 D / L + 1
            const long k0 = (b0 + tau) / rec.sps;
            const int nsym = nb > 0 ? (int)((b0 + nb - 1 + tau) / rec.sps - k0) + rec.span : 0;
            __syncthreads();      // the previous range's readers are done
            base_fill(L, a, em, rec, k0, nsym, tid);
            __syncthreads();
            unsigned sum = 0;
            for (int j = tid; j < nb; j += kCapThreads) {
                int yr, yi;
                base_y(L, rec, b0 + j + tau, k0, &yr, &yi);
                sum += (unsigned)yr * (unsigned)rec.factor;
            }
            unsigned total;
            block_scan(sum, part, tid, &total);
            if (tid == 0) a.prefix[(long)s.phase_slot * a.tiles + tile] = total;
        }
    }
}

// one work-group per PHASE emitter: its row of the workspace becomes the exclusive prefix sums over the tiles
__global__ __launch_bounds__(kCapThreads) void cap_phase_scan(unsigned* __restrict__ prefix, long tiles) {
    __shared__ unsigned part[kCapWaves];
    const int tid = threadIdx.x;
    unsigned* row = prefix + (long)blockIdx.x * tiles;
    unsigned carry = 0;
    for (long t0 = 0; t0 < tiles; t0 += kCapThreads) {
        const long t = t0 + tid;
        const unsigned own = t < tiles ? row[t] : 0u;
        unsigned total;
        const unsigned incl = block_scan(own, part, tid, &total);
        if (t < tiles) row[t] = carry + incl - own;
        carry += total;
    }
}

__global__ __launch_bounds__(kCapThreads) void cap_main(const CapArgs a, unsigned* __restrict__ out, u64* __restrict__ saturated) {
    __shared__ unsigned nco[kNcoEntries];
    __shared__ BaseLds L;
    __shared__ unsigned z[kCapMaxBase + 8];      // gated baseband samples, re | im << 16
    __shared__ short htap[kCapTapSlots];
    __shared__ unsigned part[kCapWaves];
    __shared__ unsigned live;      // bit e: emitter e is on somewhere in the tile
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < kNcoEntries; i += kCapThreads) nco[i] = d_nco[i];
    unsigned nsat = 0;
    const long half = 1l << (a.q - 1);

    for (long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        const long n0 = tile * kCapTile;
        long sr[kCapPerLane] = {}, si[kCapPerLane] = {};
        // which emitters are on anywhere in this tile: one lane per emitter decides, so the records' loads and the two 64-bit
        // divisions behind each decision run side by side, not one emitter after the other
        __syncthreads();      // the previous tile's readers of `live` are done
        if (wave == 0) {
            bool on = false;
            if (lane < a.E) {
                const ScnEmitter s = a.emitters[lane];
                int r0;
                const long b0 = tile_base(s, tile, &r0);
                on = gate_any(gate_at(s.e, b0), min(s.K + (r0 + (kCapTile - 1) * s.e.decimate) / s.e.interpolate, kCapMaxBase));
            }
            const u64 m = __ballot(on);
            if (lane == 0) live = (unsigned)m;
        }
        __syncthreads();
        unsigned todo = (unsigned)__builtin_amdgcn_readfirstlane((int)live);
        while (todo != 0) {      // uniform: every barrier inside is met by the whole work-group; a skipped emitter's mixed samples are 0
            const int em = __builtin_ctz(todo);
            todo &= todo - 1;
            const ScnEmitter s = a.emitters[em];
            const int Li = s.e.interpolate, D = s.e.decimate, T = s.e.ntaps, K = s.K;
            int r0;
            const long b0 = tile_base(s, tile, &r0);
            const int qlast = r0 + (kCapTile - 1) * D;                 // < 2^15
            const int nb = min(K + qlast / Li, kCapMaxBase);           // baseband samples b0 .. m(n0 + 1023)
            const Gate g = gate_at(s.e, b0);
            const SynClass rec = a.classes[s.e.cls];
            const unsigned ckey = syn_frame_key(a.kseed, cap_f(em + 1, kFieldConstants, 0));
            const unsigned tau = (unsigned)(((u64)syn_draw(ckey, 0) * (unsigned)rec.sps) >> 32);
            const long k0 = (b0 + tau) / rec.sps;
            const int nsym = (int)((b0 + nb - 1 + tau) / rec.sps - k0) + rec.span;
            __syncthreads();      // the table is in place; the previous emitter's readers are done
            base_fill(L, a, em, rec, k0, nsym, tid);
            const int slots = min(K * Li, kCapTapSlots);
            for (int t = tid; t < slots; t += kCapThreads) htap[t] = t < T ? a.taps[s.e.first_tap + t] : (short)0;
            __syncthreads();

            // (2) five adjacent baseband samples per thread
            int zr[kCapBasePerThread], zi[kCapBasePerThread];
            const int j0 = kCapBasePerThread * tid;
#pragma unroll
            for (int c = 0; c < kCapBasePerThread; ++c) {
                zr[c] = zi[c] = 0;
                if (j0 + c < nb) base_y(L, rec, b0 + j0 + c + tau, k0, &zr[c], &zi[c]);
            }
            if (rec.mode == MDC_SYNTH_PHASE) {      // uniform
                unsigned inc[kCapBasePerThread], own = 0;
#pragma unroll
                for (int c = 0; c < kCapBasePerThread; ++c) {
                    inc[c] = j0 + c < nb ? (unsigned)zr[c] * (unsigned)rec.factor : 0u;
                    own += inc[c];
                }
                unsigned total;
                const unsigned incl = block_scan(own, part, tid, &total);
                unsigned theta = syn_draw(ckey, 3) + a.prefix[(long)s.phase_slot * a.tiles + tile] + (incl - own);
#pragma unroll
                for (int c = 0; c < kCapBasePerThread; ++c) {
                    theta += inc[c];
                    const unsigned cs = nco[theta >> 20];
                    const int cc = (int)(short)(cs & 0xFFFFu), ss = (int)(short)(cs >> 16);
                    zr[c] = ((cc * rec.amp + 16384) >> 15) + rec.add_re;
                    zi[c] = ((ss * rec.amp + 16384) >> 15) + rec.add_im;
                }
            } else {
#pragma unroll
                for (int c = 0; c < kCapBasePerThread; ++c) {
                    zr[c] += rec.add_re;
                    zi[c] += rec.add_im;
                }
            }
#pragma unroll
            for (int c = 0; c < kCapBasePerThread; ++c)
                if (j0 + c < nb) {
                    long dwell;
                    const bool on = gate_on(g, j0 + c, &dwell);
                    z[j0 + c] = on ? ((unsigned)zr[c] & 0xFFFFu) | ((unsigned)zi[c] << 16) : 0u;
                }
            __syncthreads();

            // (3) the lane's four outputs
            const long gain = s.e.gain;
#pragma unroll
            for (int e = 0; e < kCapPerLane; ++e) {
                const int nl = kCapPerLane * tid + e;
                const unsigned qq = (unsigned)(r0 + nl * D);
                const unsigned dm = qq / (unsigned)Li, r = qq - dm * (unsigned)Li;
                const int top = (int)dm + K - 1;      // local index of z_m
                int ar = 0, ai = 0;
                for (int i = 0; i < K; ++i) {
                    const int h = htap[r + (unsigned)i * (unsigned)Li];
                    const unsigned v = z[top - i];
                    ar += h * (int)(short)(v & 0xFFFFu);
                    ai += h * (int)(short)(v >> 16);
                }
                const int vr = (ar + 16384) >> 15, vi = (ai + 16384) >> 15;
                const int ur = sat16(vr), ui = sat16(vi);
                if (n0 + nl < a.n) nsat += (ur != vr ? 1u : 0u) + (ui != vi ? 1u : 0u);
                unsigned step = s.e.phase_step[0];
                if (s.e.hops > 1) {      // uniform
                    long dwell;
                    gate_on(g, top, &dwell);
                    const unsigned hop = cap_hop(a.kseed, em, (u64)dwell, s.e.hops);
                    step = a.emitters[em].e.phase_step[hop & (kScnMaxHops - 1)];      // (from memory: a dynamic index into the copy would go to scratch)
                }
                const unsigned phi = s.e.phase0 + (unsigned)(u64)(n0 + nl) * step;
                const unsigned cs = nco[phi >> 20];
                const int cc = (int)(short)(cs & 0xFFFFu), ss = (int)(short)(cs >> 16);
                const int mr = (ur * cc - ui * ss + 32768) >> 16, mi = (ur * ss + ui * cc + 32768) >> 16;
                sr[e] += (long)mr * gain;
                si[e] += (long)mi * gain;
            }
        }

        // noise, rounding shift, dc, clamp
        const long nq = n0 + kCapPerLane * tid;      // a multiple of 4: the lane's pairs share n >> 7
        const unsigned nkey = syn_frame_key(a.kseed, cap_f(0, kFieldNoise, (u64)nq >> 7));
        unsigned o[kCapPerLane];
#pragma unroll
        for (int e = 0; e < kCapPerLane; ++e) {
            const unsigned j = kSynDrawNoise + 8u * (unsigned)((nq + e) & 127);
            long vr = sr[e], vi = si[e];
            if (a.gain_noise != 0) {      // uniform
                vr += (long)syn_gauss(nkey, j) * a.gain_noise;
                vi += (long)syn_gauss(nkey, j + 4u) * a.gain_noise;
            }
            vr = ((vr + half) >> a.q) + a.dc_re;
            vi = ((vi + half) >> a.q) + a.dc_im;
            const long cr = vr < -32768 ? -32768 : vr > 32767 ? 32767 : vr, ci = vi < -32768 ? -32768 : vi > 32767 ? 32767 : vi;
            if (nq + e < a.n) nsat += (cr != vr ? 1u : 0u) + (ci != vi ? 1u : 0u);
            o[e] = ((unsigned)cr & 0xFFFFu) | ((unsigned)ci << 16);
        }
        if (nq + kCapPerLane <= a.n) {
            const uint4 v = make_uint4(o[0], o[1], o[2], o[3]);
            __builtin_memcpy(out + nq, &v, sizeof(v));
        } else {
#pragma unroll
            for (int e = 0; e < kCapPerLane; ++e)
                if (nq + e < a.n) out[nq + e] = o[e];
        }
    }
    if (saturated == nullptr) return;      // uniform over the grid
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) nsat += __shfl_xor(nsat, d, 64);
    __syncthreads();
    if (lane == 0) part[wave] = nsat;
    __syncthreads();
    if (tid == 0) {
        u64 sum = 0;
#pragma unroll
        for (int w = 0; w < kCapWaves; ++w) sum += part[w];
        if (sum != 0) atomicAdd(saturated, sum);
    }
}

int64_t scene_bytes_of(int32_t E, int64_t ntaps) {
    return round16(round16((int64_t)sizeof(ScnHeader) + (int64_t)E * (int64_t)sizeof(ScnEmitter)) + 2 * ntaps);
}

// a call's check of a scene blob, on the host copy; on success h holds the header
int scene_open(const char* who, const void* scene_host, int64_t scene_bytes, ScnHeader& h) {
    if (!scene_host) { set_error("%s: null scene", who); return MDC_EINVAL; }
    if (scene_bytes < (int64_t)sizeof(ScnHeader)) { set_error("%s: scene_bytes is %lld, smaller than a scene's header", who, (long long)scene_bytes); return MDC_EINVAL; }
    memcpy(&h, scene_host, sizeof h);
    if (h.magic != kScnMagic || h.version != kScnVersion) { set_error("%s: scene_host does not hold a scene of mdc_iq_synth_scene", who); return MDC_EINVAL; }
    if (h.bytes != scene_bytes) { set_error("%s: scene_bytes is %lld, the scene holds %lld bytes", who, (long long)scene_bytes, (long long)h.bytes); return MDC_EINVAL; }
    if (h.E < 0 || h.E > kScnMaxEmitters || h.q < 1 || h.q > kSynMaxQ || h.gain_noise < 0 || h.nphase < 0 || h.nphase > h.E || h.ntaps < 0 ||
        h.dc_re < -32768 || h.dc_re > 32767 || h.dc_im < -32768 || h.dc_im > 32767 || h.off_emitters != (int64_t)sizeof(ScnHeader) ||
        h.off_taps != round16(h.off_emitters + (int64_t)h.E * (int64_t)sizeof(ScnEmitter)) || h.bytes != scene_bytes_of(h.E, h.ntaps)) {
        set_error("%s: the scene's header is damaged", who);
        return MDC_EINVAL;
    }
    return MDC_OK;
}

// one emitter record against the plan's classes and the scene's taps; slot counts the PHASE emitters
int emitter_check(const char* who, int k, const mdc_iq_synth_emitter& e, const void* plan_host, const SynHeader& ph, const int16_t* taps,
                  int64_t ntaps, ScnEmitter& out, int32_t& nphase) {
    if (e.reserved[0] != 0 || e.reserved[1] != 0) { set_error("%s: emitter %d: reserved must be 0", who, k); return MDC_EINVAL; }
    if (e.cls < 0 || e.cls >= ph.C) { set_error("%s: emitter %d: cls must be in 0..%d, the plan's classes (got %d)", who, k, ph.C - 1, e.cls); return MDC_EINVAL; }
    if (e.interpolate < 1 || e.interpolate > kScnMaxL) { set_error("%s: emitter %d: interpolate must be in 1..%d (got %d)", who, k, kScnMaxL, e.interpolate); return MDC_EINVAL; }
    if (e.decimate < 1 || e.decimate > e.interpolate) {
        set_error("%s: emitter %d: decimate must be in 1..interpolate = %d, an emitter is never decimated (got %d)", who, k, e.interpolate, e.decimate);
        return MDC_EINVAL;
    }
    if (e.ntaps < 1 || e.ntaps > kScnMaxTaps) { set_error("%s: emitter %d: ntaps must be in 1..%d (got %d)", who, k, kScnMaxTaps, e.ntaps); return MDC_EINVAL; }
    if (e.first_tap < 0 || (int64_t)e.first_tap + e.ntaps > ntaps) {
        set_error("%s: emitter %d: taps %d .. %lld lie outside the %lld taps given", who, k, e.first_tap, (long long)e.first_tap + e.ntaps - 1, (long long)ntaps);
        return MDC_EINVAL;
    }
    const int K = (e.ntaps + e.interpolate - 1) / e.interpolate;
    if (K > kScnMaxBranch) {
        set_error("%s: emitter %d: a branch holds ceil(ntaps / interpolate) = %d taps, more than %d", who, k, K, kScnMaxBranch);
        return MDC_EINVAL;
    }
    for (int r = 0; r < e.interpolate; ++r) {
        int64_t sum = 0;
        for (int t = r; t < e.ntaps; t += e.interpolate) sum += taps[e.first_tap + t] < 0 ? -(int64_t)taps[e.first_tap + t] : taps[e.first_tap + t];
        if (sum > kScnMaxBranchAbsSum) {
            set_error("%s: emitter %d: the taps of branch %d (h[%d], h[%d + %d], ...) sum to %lld in absolute value: more than 65535", who, k, r, r, r,
                      e.interpolate, (long long)sum);
            return MDC_EINVAL;
        }
    }
    if (e.hops < 1 || e.hops > kScnMaxHops) { set_error("%s: emitter %d: hops must be in 1..%d (got %d)", who, k, kScnMaxHops, e.hops); return MDC_EINVAL; }
    if (e.start < 0 || e.on < 0 || e.period < 0 || e.start > kScnMaxTime || e.on > kScnMaxTime || e.period > kScnMaxTime) {
        set_error("%s: emitter %d: start, on and period must be in 0..2^52 (got %lld, %lld, %lld)", who, k, (long long)e.start, (long long)e.on,
                  (long long)e.period);
        return MDC_EINVAL;
    }
    if (e.hops > 1 && e.period == 0) { set_error("%s: emitter %d: %d hops need a period > 0: a dwell is one period", who, k, e.hops); return MDC_EINVAL; }
    SynClass c;
    memcpy(&c, static_cast<const unsigned char*>(plan_host) + ph.off_classes + (int64_t)e.cls * (int64_t)sizeof c, sizeof c);
    out.e = e;
    out.K = K;
    out.phase_slot = c.mode == MDC_SYNTH_PHASE ? nphase++ : -1;
    return MDC_OK;
}

}  // namespace

}  // namespace mdc

using namespace mdc;

int64_t mdc_iq_synth_scene_bytes(int32_t nemitters, int64_t ntaps) {
    static const char who[] = "mdc_iq_synth_scene_bytes";
    if (nemitters < 0 || nemitters > kScnMaxEmitters) { set_error("%s: nemitters must be in 0..%d (got %d)", who, kScnMaxEmitters, nemitters); return MDC_EINVAL; }
    if (ntaps < 0 || ntaps > (int64_t)kScnMaxEmitters * kScnMaxTaps) {
        set_error("%s: ntaps must be in 0..%d (got %lld)", who, kScnMaxEmitters * kScnMaxTaps, (long long)ntaps);
        return MDC_EINVAL;
    }
    return scene_bytes_of(nemitters, ntaps);
}

int mdc_iq_synth_scene(const void* plan_host, int64_t plan_bytes, const mdc_iq_synth_emitter* emitters_host, int32_t nemitters,
                       const int16_t* taps_host, int64_t ntaps, int32_t gain_noise, int32_t q, int16_t dc_re, int16_t dc_im, void* scene_host,
                       int64_t scene_bytes) {
    static const char who[] = "mdc_iq_synth_scene";
    return guarded(who, [&]() -> int {
        SynHeader ph;
        int rc = syn_plan_open(who, plan_host, plan_bytes, ph);
        if (rc != MDC_OK) return rc;
        if ((rc = syn_plan_classes_check(who, plan_host, ph)) != MDC_OK) return rc;
        if (nemitters < 0 || nemitters > kScnMaxEmitters) {
            set_error("%s: emitter %d: a scene holds at most %d emitters (got %d)", who, kScnMaxEmitters, kScnMaxEmitters, nemitters);
            return MDC_EINVAL;
        }
        if (nemitters > 0 && !emitters_host) { set_error("%s: null emitters", who); return MDC_EINVAL; }
        if (ntaps < 0 || ntaps > (int64_t)kScnMaxEmitters * kScnMaxTaps || (ntaps > 0 && !taps_host)) {
            set_error("%s: ntaps must be in 0..%d with a tap array (got %lld)", who, kScnMaxEmitters * kScnMaxTaps, (long long)ntaps);
            return MDC_EINVAL;
        }
        if (gain_noise < 0) { set_error("%s: gain_noise must be >= 0 (got %d)", who, gain_noise); return MDC_EINVAL; }
        if (q < 1 || q > kSynMaxQ) { set_error("%s: q must be in 1..%d (got %d)", who, kSynMaxQ, q); return MDC_EINVAL; }
        ScnHeader h{};
        h.magic = kScnMagic;
        h.version = kScnVersion;
        h.E = nemitters;
        h.q = q;
        h.gain_noise = gain_noise;
        h.dc_re = dc_re;
        h.dc_im = dc_im;
        h.ntaps = ntaps;
        h.off_emitters = (int64_t)sizeof(ScnHeader);
        h.off_taps = round16(h.off_emitters + (int64_t)nemitters * (int64_t)sizeof(ScnEmitter));
        h.bytes = scene_bytes_of(nemitters, ntaps);
        std::vector<ScnEmitter> em((size_t)nemitters);
        for (int32_t k = 0; k < nemitters; ++k) {
            em[(size_t)k] = ScnEmitter{};
            if ((rc = emitter_check(who, k, emitters_host[k], plan_host, ph, taps_host, ntaps, em[(size_t)k], h.nphase)) != MDC_OK) return rc;
        }
        if (scene_bytes != h.bytes) {
            set_error("%s: scene_bytes is %lld, mdc_iq_synth_scene_bytes gives %lld", who, (long long)scene_bytes, (long long)h.bytes);
            return MDC_EINVAL;
        }
        if (!scene_host) { set_error("%s: null scene buffer", who); return MDC_EINVAL; }
        unsigned char* blob = static_cast<unsigned char*>(scene_host);
        memset(blob, 0, (size_t)h.bytes);
        memcpy(blob, &h, sizeof h);
        if (nemitters) memcpy(blob + h.off_emitters, em.data(), (size_t)nemitters * sizeof(ScnEmitter));
        if (ntaps) memcpy(blob + h.off_taps, taps_host, 2 * (size_t)ntaps);
        return MDC_OK;
    });
}

int mdc_iq_synth_scene_hops(const void* scene_host, int64_t scene_bytes, uint64_t seed, int32_t emitter, int64_t first_dwell, int64_t n,
                            int32_t* hop_index_out) {
    static const char who[] = "mdc_iq_synth_scene_hops";
    ScnHeader h;
    const int rc = scene_open(who, scene_host, scene_bytes, h);
    if (rc != MDC_OK) return rc;
    if (emitter < 0 || emitter >= h.E) { set_error("%s: emitter must be in 0..%d (got %d)", who, h.E - 1, emitter); return MDC_EINVAL; }
    if (first_dwell < 0 || n < 0 || first_dwell > kScnMaxTime || n > kScnMaxTime) {
        set_error("%s: first_dwell and n must be in 0..2^52 (got %lld, %lld)", who, (long long)first_dwell, (long long)n);
        return MDC_EINVAL;
    }
    if (n == 0) return MDC_OK;
    if (!hop_index_out) { set_error("%s: null output", who); return MDC_EINVAL; }
    ScnEmitter s;
    memcpy(&s, static_cast<const unsigned char*>(scene_host) + h.off_emitters + (int64_t)emitter * (int64_t)sizeof s, sizeof s);
    const unsigned kseed = syn_seed_key(seed);
    for (int64_t i = 0; i < n; ++i) hop_index_out[i] = (int32_t)cap_hop(kseed, emitter, (u64)(first_dwell + i), s.e.hops);
    return MDC_OK;
}

int64_t mdc_iq_synth_capture_workspace_bytes(const void* scene_host, int64_t scene_bytes, int64_t n_pairs) {
    static const char who[] = "mdc_iq_synth_capture_workspace_bytes";
    ScnHeader h;
    const int rc = scene_open(who, scene_host, scene_bytes, h);
    if (rc != MDC_OK) return rc;
    if (n_pairs < 0 || n_pairs > kCapMaxPairs) { set_error("%s: n_pairs must be in 0..2^34 (got %lld)", who, (long long)n_pairs); return MDC_EINVAL; }
    return round16(4 * (int64_t)h.nphase * ((n_pairs + kCapTile - 1) / kCapTile));
}

int mdc_iq_synth_capture(const void* scene_host, const void* scene_dev, int64_t scene_bytes, const void* plan_host, const void* plan_dev,
                         int64_t plan_bytes, uint64_t seed, int64_t n_pairs, int16_t* out_dev, uint64_t* saturated_dev, void* workspace_dev,
                         int64_t workspace_bytes, void* hip_stream) {
    static const char who[] = "mdc_iq_synth_capture";
    ScnHeader h;
    SynHeader ph;
    int rc = scene_open(who, scene_host, scene_bytes, h);
    if (rc != MDC_OK) return rc;
    if ((rc = syn_plan_open(who, plan_host, plan_bytes, ph)) != MDC_OK) return rc;
    if (n_pairs < 0 || n_pairs > kCapMaxPairs) { set_error("%s: n_pairs must be in 0..2^34 (got %lld)", who, (long long)n_pairs); return MDC_EINVAL; }
    if ((rc = iq_aligned(who, "output", out_dev, 4)) != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "saturated_dev", saturated_dev, 8)) != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "plan_dev", plan_dev, 8)) != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "scene_dev", scene_dev, 8)) != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "workspace_dev", workspace_dev, 4)) != MDC_OK) return rc;
    const int64_t tiles = (n_pairs + kCapTile - 1) / kCapTile;
    const int64_t need = round16(4 * (int64_t)h.nphase * tiles);
    if (workspace_bytes < need) {
        set_error("%s: workspace_bytes is %lld, mdc_iq_synth_capture_workspace_bytes gives %lld", who, (long long)workspace_bytes, (long long)need);
        return MDC_EINVAL;
    }
    if ((rc = syn_plan_classes_check(who, plan_host, ph)) != MDC_OK) return rc;
    // the emitter records' indices are checked here, on the host copy: the kernels read the classes and taps they name
    int32_t nphase = 0;
    for (int32_t k = 0; k < h.E; ++k) {
        ScnEmitter s;
        memcpy(&s, static_cast<const unsigned char*>(scene_host) + h.off_emitters + (int64_t)k * (int64_t)sizeof s, sizeof s);
        const mdc_iq_synth_emitter& e = s.e;
        bool ok = e.cls >= 0 && e.cls < ph.C && e.interpolate >= 1 && e.interpolate <= kScnMaxL && e.decimate >= 1 && e.decimate <= e.interpolate &&
                  e.ntaps >= 1 && e.ntaps <= kScnMaxTaps && e.first_tap >= 0 && (int64_t)e.first_tap + e.ntaps <= h.ntaps && e.hops >= 1 &&
                  e.hops <= kScnMaxHops && e.start >= 0 && e.on >= 0 && e.period >= 0 && e.start <= kScnMaxTime && e.on <= kScnMaxTime &&
                  e.period <= kScnMaxTime && (e.hops == 1 || e.period > 0);
        if (ok) {
            SynClass c;
            memcpy(&c, static_cast<const unsigned char*>(plan_host) + ph.off_classes + (int64_t)e.cls * (int64_t)sizeof c, sizeof c);
            ok = s.K == (e.ntaps + e.interpolate - 1) / e.interpolate && s.K <= kScnMaxBranch &&
                 s.phase_slot == (c.mode == MDC_SYNTH_PHASE ? nphase++ : -1);
        }
        if (!ok) { set_error("%s: the scene's record of emitter %d is damaged, or the scene was built for another plan", who, k); return MDC_EINVAL; }
    }
    if (nphase != h.nphase) { set_error("%s: the scene's header is damaged", who); return MDC_EINVAL; }
    if (n_pairs == 0) return MDC_OK;
    if (!out_dev || !plan_dev || !scene_dev || (need > 0 && !workspace_dev)) { set_error("%s: null buffer", who); return MDC_EINVAL; }
    const unsigned char* pd = static_cast<const unsigned char*>(plan_dev);
    const unsigned char* sd = static_cast<const unsigned char*>(scene_dev);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return guarded(who, [&]() -> int {
        CapArgs a{};
        a.emitters = reinterpret_cast<const ScnEmitter*>(sd + h.off_emitters);
        a.taps = reinterpret_cast<const short*>(sd + h.off_taps);
        a.classes = reinterpret_cast<const SynClass*>(pd + ph.off_classes);
        a.points = reinterpret_cast<const unsigned*>(pd + ph.off_points);
        a.ptaps = reinterpret_cast<const unsigned*>(pd + ph.off_taps);
        a.prefix = static_cast<unsigned*>(workspace_dev);
        a.n = (long)n_pairs;
        a.tiles = (long)tiles;
        a.kseed = syn_seed_key(seed);
        a.E = h.E;
        a.q = h.q;
        a.gain_noise = h.gain_noise;
        a.dc_re = h.dc_re;
        a.dc_im = h.dc_im;
        const dim3 grid((unsigned)(tiles < kCapGridCap ? tiles : kCapGridCap));
        if (h.nphase > 0) {
            hipLaunchKernelGGL(cap_phase_sums, grid, dim3(kCapThreads), 0, s, a);
            MDC_HIP(hipGetLastError());
            hipLaunchKernelGGL(cap_phase_scan, dim3((unsigned)h.nphase), dim3(kCapThreads), 0, s, a.prefix, a.tiles);
            MDC_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(cap_main, grid, dim3(kCapThreads), 0, s, a, reinterpret_cast<unsigned*>(out_dev), reinterpret_cast<u64*>(saturated_dev));
        MDC_HIP(hipGetLastError());
        return MDC_OK;
    });
}
