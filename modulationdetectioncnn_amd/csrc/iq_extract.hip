// mdc_iq_extract -- K stretches of one capture through mdc_iq_resample's chain (tune, low-pass, resample by L / D; exact
// integers) in ONE launch, each stretch with its own oscillator, factors and filter (include/mdc.h, "batched extraction").  The
// numpy restatement is tests/iq_resample_ref.py applied to each job's slice.
//
//   job       a stretch [first_pair, first_pair + pairs) of the capture, (phase0, phase_step), a filter index, and the range
//             [out_first, out_first + n_out) of the output it fills with the FIRST n_out outputs a call of mdc_iq_resample on the
//             slice would give.  The slice's semantics are had by handing the shared stages the slice: mix_tile gets the base
//             pointer iq + first_pair and the bound `pairs`, so the oscillator counts from the job's first pair and everything at
//             or beyond the job's last pair is written into LDS as zeros, whatever the capture holds there.
//   tile      the resampler's, per filter (iq_resample.hip, iq_resample_plan.h): tile t of a job is its outputs t q L on, which
//             start at the job's pair t q D exactly and at branch 0 -- 32-bit local arithmetic inside a tile.  The planner lists
//             every (job, tile) of the plan; work-groups stride over that list (grid cap kResGridCap).  The list is ordered by
//             (parity, filter, job, tile): the tiles of one filter are adjacent.
//   taps      per FILTER, so they cannot be kernel arguments: the planner writes every filter's branch-major image (the one
//             resample_plan builds: odd branch stride, groups of kResTapGroup dwords) into the plan blob, and a work-group copies
//             the image of its tile's filter into LDS -- only when the filter differs from the one it holds.  That test is
//             uniform over the work-group (it depends on the tile record alone), the copy sits between the two barriers every
//             thread reaches, and the second barrier publishes it together with the mixed samples.
//   stages    mix_tile and fir_output of iq_mix.h, called, not copied (the resampler's private copies bought it 6 %; whether
//             they would buy anything here: DESIGN.md 5.22).  Whether a filter's outputs can start on an odd local sample (ODD:
//             the v_alignbit path of fir_output) is a property of (L, D); the kernel holds both instantiations of the filter
//             loop and takes one per tile, a branch that is uniform over the work-group.
// LDS: the resampler's 4096 + 768 + 2 * 4241 dwords (52.1 KiB).  The call only enqueues; vector memory for every store; no
// work-group waits on another.
#include "iq_resample_plan.h"

#include <algorithm>
#include <cstring>

namespace mdc {

namespace {

constexpr uint32_t kExtMagic = 0x5845434Du;      // "MCEX"
constexpr uint32_t kExtVersion = 1;

// the blob: ExtHeader | jobs (mdc_iq_extract_job) | filters (ExtFilter) | tap images (dwords) | tiles (ExtTile); every part starts
// on a multiple of 16 bytes, all offsets are from the blob's first byte
struct ExtHeader {
    uint32_t magic, version;
    int32_t format, nfilters;
    int64_t njobs, ntiles, pairs_in, out_pairs, bytes;
    int64_t off_jobs, off_filters, off_images, off_tiles;
    int64_t reserved;
};
struct ExtFilter {
    int32_t L, D, ngroups, stride, tapdw, tile_out, tile_in, odd;
    int32_t image;          // the filter's first dword in the tap images
    int32_t ntaps, pad[2];
};
struct ExtTile { int32_t job, tile; };
static_assert(sizeof(ExtHeader) == 96 && sizeof(ExtFilter) == 48 && sizeof(ExtTile) == 8 && sizeof(mdc_iq_extract_job) == 48 &&
              sizeof(mdc_iq_extract_filter) == 16, "the plan blob's records");

constexpr int64_t kExtMaxJobs = (int64_t)1 << 24, kExtMaxTiles = (int64_t)1 << 28;      // the tile list stays below 2 GiB

template <bool ODD>
__device__ __forceinline__ void extract_filter_tile(const unsigned* re, const unsigned* im, const unsigned* tl, const ExtFilter& f, int nout,
                                                    unsigned* __restrict__ o, int tid) {
    const unsigned L = (unsigned)f.L, D = (unsigned)f.D;
    for (int j = tid; j < nout; j += kResThreads) {
        const unsigned jd = (unsigned)j * D;                     // < tile_in * L <= 2^18
        const unsigned start = (jd + L - 1) / L, branch = start * L - jd;
        const unsigned* tp = tl + branch * (unsigned)f.stride;
        o[j] = fir_output<ODD, kResTapGroup>(re, im, (int)(start >> 1), (start & 1u) << 4, f.ngroups, [&](int k) { return tp[k]; });
    }
}

template <int FMT>
__global__ __launch_bounds__(kResThreads) void iq_extract_kernel(const unsigned char* __restrict__ iq, const mdc_iq_extract_job* __restrict__ jobs,
                                                                 const ExtFilter* __restrict__ filters, const unsigned* __restrict__ images,
                                                                 const ExtTile* __restrict__ tiles, long ntiles, unsigned* __restrict__ out) {
    __shared__ unsigned lds[kNcoEntries + kResTapDwords + 2 * kPlaneDwords];
    unsigned* nco = lds;
    unsigned* tl = lds + kNcoEntries;
    unsigned* re = tl + kResTapDwords;
    unsigned* im = re + kPlaneDwords;
    const int tid = threadIdx.x;
    for (int i = tid; i < kNcoEntries; i += kResThreads) nco[i] = d_nco[i];
    int held = -1;      // the filter whose image is in LDS

    for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const ExtTile w = tiles[t];
        const mdc_iq_extract_job jb = jobs[w.job];
        const ExtFilter f = filters[jb.filter];
        const long out0 = (long)w.tile * f.tile_out, in0 = (long)w.tile * f.tile_in;
        const long left = jb.n_out - out0;
        const int nout = left < f.tile_out ? (int)left : f.tile_out;
        // local pairs the filter reads: the last output's start, its branch's tap groups, one more dword for the ODD look-ahead
        const int last = (int)(((unsigned)(nout - 1) * (unsigned)f.D + (unsigned)f.L - 1) / (unsigned)f.L);
        const int span = last + 2 * kResTapGroup * f.ngroups + 2;      // <= kIqTilePairs + 9
        const int quads = (span + 3) >> 2;
        __syncthreads();      // the table is in place; the previous tile's filter has read its samples and its taps
        if (jb.filter != held) {      // uniform over the work-group
            const unsigned* img = images + f.image;
            for (int i = tid; i < f.tapdw; i += kResThreads) tl[i] = img[i];
            held = jb.filter;
        }
        mix_tile<FMT>(iq + jb.first_pair * Quad<FMT>::kPairBytes, in0, jb.pairs, jb.phase0, jb.phase_step, quads, nco, re, im, tid);
        __syncthreads();
        unsigned* o = out + jb.out_first + out0;
        if (f.odd) extract_filter_tile<true>(re, im, tl, f, nout, o, tid);
        else       extract_filter_tile<false>(re, im, tl, f, nout, o, tid);
    }
}

int64_t round16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// what both planner entries check of the filters' shapes and of each job by itself; on success the geometry of every filter, the
// tiles of every job and the blob's layout
struct ExtLayout {
    std::vector<ResPlan> geo;
    std::vector<int64_t> job_tiles;
    ExtHeader h{};
};

int extract_layout(const char* who, int64_t njobs, int32_t nfilters, const mdc_iq_extract_job* jobs, const mdc_iq_extract_filter* filters,
                   ExtLayout& lay) {
    if (njobs < 0 || njobs > kExtMaxJobs) { set_error("%s: njobs must be in 0..%lld (got %lld)", who, (long long)kExtMaxJobs, (long long)njobs); return MDC_EINVAL; }
    if (nfilters < 0) { set_error("%s: negative nfilters", who); return MDC_EINVAL; }
    if ((njobs > 0 && !jobs) || (nfilters > 0 && !filters)) { set_error("%s: null jobs or filters", who); return MDC_EINVAL; }
    lay.geo.resize((size_t)nfilters);
    int64_t image_dwords = 0;
    for (int32_t k = 0; k < nfilters; ++k) {
        const mdc_iq_extract_filter& f = filters[k];
        char name[64];
        snprintf(name, sizeof name, "%s: filter %d", who, k);
        const int rc = resample_shape_check(name, 0, f.ntaps, f.interpolate, f.decimate);
        if (rc != MDC_OK) return rc;
        if (!resample_geometry(f.interpolate, f.decimate, f.ntaps, lay.geo[(size_t)k])) {
            set_error("%s: internal: the branch-major tap image exceeds %d dwords", name, kResTapDwords);
            return MDC_EINVAL;
        }
        image_dwords += lay.geo[(size_t)k].tapdw;
    }
    lay.job_tiles.resize((size_t)njobs);
    int64_t ntiles = 0;
    for (int64_t j = 0; j < njobs; ++j) {
        const mdc_iq_extract_job& b = jobs[j];
        if (b.reserved != 0) { set_error("%s: job %lld: reserved must be 0 (got %d)", who, (long long)j, b.reserved); return MDC_EINVAL; }
        if (b.filter < 0 || b.filter >= nfilters) {
            set_error("%s: job %lld: filter index %d is not in 0..%d", who, (long long)j, b.filter, nfilters - 1);
            return MDC_EINVAL;
        }
        if (b.first_pair < 0 || b.pairs < 0 || b.pairs > ((int64_t)1 << 58) || b.first_pair > ((int64_t)1 << 58)) {
            set_error("%s: job %lld: first_pair and pairs must be in 0..2^58 (got %lld, %lld)", who, (long long)j, (long long)b.first_pair, (long long)b.pairs);
            return MDC_EINVAL;
        }
        const mdc_iq_extract_filter& f = filters[b.filter];
        const int64_t most = resample_out_count(b.pairs, f.ntaps, f.interpolate, f.decimate);
        if (b.n_out < 0 || b.n_out > most) {
            set_error("%s: job %lld: n_out is %lld, its %lld pairs give at most %lld outputs (mdc_iq_resample_out_count)", who, (long long)j,
                      (long long)b.n_out, (long long)b.pairs, (long long)most);
            return MDC_EINVAL;
        }
        const int tile_out = lay.geo[(size_t)b.filter].tile_out;
        lay.job_tiles[(size_t)j] = (b.n_out + tile_out - 1) / tile_out;
        ntiles += lay.job_tiles[(size_t)j];
        if (ntiles > kExtMaxTiles) { set_error("%s: job %lld: more than %lld tiles in one plan", who, (long long)j, (long long)kExtMaxTiles); return MDC_EINVAL; }
    }
    ExtHeader& h = lay.h;
    h.magic = kExtMagic;
    h.version = kExtVersion;
    h.nfilters = nfilters;
    h.njobs = njobs;
    h.ntiles = ntiles;
    h.off_jobs = (int64_t)sizeof(ExtHeader);
    h.off_filters = h.off_jobs + njobs * (int64_t)sizeof(mdc_iq_extract_job);
    h.off_images = h.off_filters + (int64_t)nfilters * (int64_t)sizeof(ExtFilter);
    h.off_tiles = round16(h.off_images + 4 * image_dwords);
    h.bytes = round16(h.off_tiles + ntiles * (int64_t)sizeof(ExtTile));
    return MDC_OK;
}

template <int FMT>
int extract_launch(const unsigned char* iq, const unsigned char* plan_dev, const ExtHeader& h, int16_t* out, hipStream_t s) {
    const long ntiles = (long)h.ntiles;
    const dim3 g((unsigned)(ntiles < kResGridCap ? ntiles : kResGridCap)), b(kResThreads);
    hipLaunchKernelGGL((iq_extract_kernel<FMT>), g, b, 0, s, iq, reinterpret_cast<const mdc_iq_extract_job*>(plan_dev + h.off_jobs),
                       reinterpret_cast<const ExtFilter*>(plan_dev + h.off_filters), reinterpret_cast<const unsigned*>(plan_dev + h.off_images),
                       reinterpret_cast<const ExtTile*>(plan_dev + h.off_tiles), ntiles, reinterpret_cast<unsigned*>(out));
    MDC_HIP(hipGetLastError());
    return MDC_OK;
}

}  // namespace

}  // namespace mdc

using namespace mdc;

int64_t mdc_iq_extract_plan_bytes(int64_t njobs, int32_t nfilters, const mdc_iq_extract_job* jobs_host, const mdc_iq_extract_filter* filters_host) {
    int64_t bytes = MDC_EINVAL;
    const int rc = guarded("mdc_iq_extract_plan_bytes", [&]() -> int {
        ExtLayout lay;
        const int r = extract_layout("mdc_iq_extract_plan_bytes", njobs, nfilters, jobs_host, filters_host, lay);
        if (r == MDC_OK) bytes = lay.h.bytes;
        return r;
    });
    return rc != MDC_OK ? (int64_t)rc : bytes;
}

int mdc_iq_extract_plan(int format, int64_t pairs_in, const mdc_iq_extract_job* jobs_host, int64_t njobs, const mdc_iq_extract_filter* filters_host,
                        int32_t nfilters, const int16_t* taps_host, int64_t ntaps_total, int64_t out_pairs, void* plan_host, int64_t plan_bytes) {
    static const char who[] = "mdc_iq_extract_plan";
    int rc = iq_format_known(who, format);
    if (rc != MDC_OK) return rc;
    if (pairs_in < 0 || pairs_in > ((int64_t)1 << 58)) { set_error("%s: pairs_in must be in 0..2^58", who); return MDC_EINVAL; }
    if (out_pairs < 0) { set_error("%s: negative out_pairs", who); return MDC_EINVAL; }
    if (ntaps_total < 0 || (ntaps_total > 0 && !taps_host)) { set_error("%s: null taps", who); return MDC_EINVAL; }
    return guarded(who, [&]() -> int {
        ExtLayout lay;
        int r = extract_layout(who, njobs, nfilters, jobs_host, filters_host, lay);
        if (r != MDC_OK) return r;
        for (int32_t k = 0; k < nfilters; ++k) {
            const mdc_iq_extract_filter& f = filters_host[k];
            if (f.first_tap < 0 || (int64_t)f.first_tap + f.ntaps > ntaps_total) {
                set_error("%s: filter %d: taps %d .. %lld lie outside the %lld taps given", who, k, f.first_tap, (long long)f.first_tap + f.ntaps - 1,
                          (long long)ntaps_total);
                return MDC_EINVAL;
            }
            long sum = 0;
            const int over = resample_branch_over(taps_host + f.first_tap, f.ntaps, f.interpolate, &sum);
            if (over) {
                set_error("%s: filter %d: the absolute values of branch %d of the taps (h[%d], h[%d + %d], ...) sum to %ld; at most 65535 keeps the "
                          "32-bit accumulation exact", who, k, over - 1, over - 1, over - 1, f.interpolate, sum);
                return MDC_EINVAL;
            }
        }
        std::vector<int64_t> order;      // the jobs that write something, by where
        for (int64_t j = 0; j < njobs; ++j) {
            const mdc_iq_extract_job& b = jobs_host[j];
            if (b.first_pair > pairs_in || b.pairs > pairs_in - b.first_pair) {
                set_error("%s: job %lld: the stretch [%lld, %lld) ends beyond the capture's %lld pairs", who, (long long)j, (long long)b.first_pair,
                          (long long)(b.first_pair + b.pairs), (long long)pairs_in);
                return MDC_EINVAL;
            }
            if (b.out_first < 0 || b.out_first > out_pairs || b.n_out > out_pairs - b.out_first) {
                set_error("%s: job %lld: the output range [%lld, %lld + %lld) is not inside the %lld output pairs", who, (long long)j, (long long)b.out_first,
                          (long long)b.out_first, (long long)b.n_out, (long long)out_pairs);
                return MDC_EINVAL;
            }
            if (b.n_out > 0) order.push_back(j);
        }
        std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
            return jobs_host[a].out_first != jobs_host[b].out_first ? jobs_host[a].out_first < jobs_host[b].out_first : a < b; });
        for (size_t i = 1; i < order.size(); ++i) {
            const mdc_iq_extract_job &p = jobs_host[order[i - 1]], &c = jobs_host[order[i]];
            if (p.out_first + p.n_out > c.out_first) {
                set_error("%s: job %lld: its output range [%lld, %lld) overlaps that of job %lld, [%lld, %lld)", who, (long long)order[i],
                          (long long)c.out_first, (long long)(c.out_first + c.n_out), (long long)order[i - 1], (long long)p.out_first,
                          (long long)(p.out_first + p.n_out));
                return MDC_EINVAL;
            }
        }
        ExtHeader& h = lay.h;
        if (plan_bytes != h.bytes) {
            set_error("%s: plan_bytes is %lld, mdc_iq_extract_plan_bytes gives %lld", who, (long long)plan_bytes, (long long)h.bytes);
            return MDC_EINVAL;
        }
        if (!plan_host) { set_error("%s: null plan buffer", who); return MDC_EINVAL; }
        h.format = format;
        h.pairs_in = pairs_in;
        h.out_pairs = out_pairs;
        unsigned char* blob = static_cast<unsigned char*>(plan_host);
        memset(blob, 0, (size_t)h.bytes);
        memcpy(blob, &h, sizeof h);
        if (njobs) memcpy(blob + h.off_jobs, jobs_host, (size_t)njobs * sizeof(mdc_iq_extract_job));
        int32_t image = 0;
        for (int32_t k = 0; k < nfilters; ++k) {
            const mdc_iq_extract_filter& f = filters_host[k];
            ResPlan p{};
            std::vector<unsigned> pk((size_t)lay.geo[(size_t)k].tapdw, 0u);
            resample_plan(f.interpolate, f.decimate, taps_host + f.first_tap, f.ntaps, p, pk.data());
            const ExtFilter e{p.L, p.D, p.ngroups, p.stride, p.tapdw, p.tile_out, p.tile_in, p.odd ? 1 : 0, image, f.ntaps, {0, 0}};
            memcpy(blob + h.off_filters + (int64_t)k * (int64_t)sizeof e, &e, sizeof e);
            memcpy(blob + h.off_images + 4 * (int64_t)image, pk.data(), 4 * pk.size());
            image += p.tapdw;
        }
        // the work items: by (parity, filter, job), a job's tiles in order
        std::vector<int64_t> by;
        for (int64_t j = 0; j < njobs; ++j)
            if (lay.job_tiles[(size_t)j] > 0) by.push_back(j);
        auto key = [&](int64_t j) { return std::make_pair(lay.geo[(size_t)jobs_host[j].filter].odd ? 1 : 0, jobs_host[j].filter); };
        std::sort(by.begin(), by.end(), [&](int64_t a, int64_t b) { return key(a) != key(b) ? key(a) < key(b) : a < b; });
        ExtTile* tiles = reinterpret_cast<ExtTile*>(blob + h.off_tiles);
        int64_t at = 0;
        for (int64_t j : by)
            for (int64_t t = 0; t < lay.job_tiles[(size_t)j]; ++t) tiles[at++] = ExtTile{(int32_t)j, (int32_t)t};
        return MDC_OK;
    });
}

int mdc_iq_extract(const void* iq_dev, int format, int64_t pairs_in, const void* plan_host, const void* plan_dev, int64_t plan_bytes, int16_t* out_dev,
                   int64_t out_pairs, void* hip_stream) {
    static const char who[] = "mdc_iq_extract";
    int rc = iq_format_known(who, format);
    if (rc != MDC_OK) return rc;
    if (!plan_host) { set_error("%s: null plan", who); return MDC_EINVAL; }
    if (plan_bytes < (int64_t)sizeof(ExtHeader)) { set_error("%s: plan_bytes is %lld, smaller than a plan's header", who, (long long)plan_bytes); return MDC_EINVAL; }
    ExtHeader h;
    memcpy(&h, plan_host, sizeof h);
    if (h.magic != kExtMagic || h.version != kExtVersion) { set_error("%s: plan_host does not hold a plan of mdc_iq_extract_plan", who); return MDC_EINVAL; }
    if (h.bytes != plan_bytes) { set_error("%s: plan_bytes is %lld, the plan holds %lld bytes", who, (long long)plan_bytes, (long long)h.bytes); return MDC_EINVAL; }
    const int64_t images_end = h.off_tiles, tiles_end = h.off_tiles + h.ntiles * (int64_t)sizeof(ExtTile);
    if (h.njobs < 0 || h.nfilters < 0 || h.ntiles < 0 || h.ntiles > kExtMaxTiles || h.off_jobs != (int64_t)sizeof(ExtHeader) ||
        h.off_filters != h.off_jobs + h.njobs * (int64_t)sizeof(mdc_iq_extract_job) ||
        h.off_images != h.off_filters + (int64_t)h.nfilters * (int64_t)sizeof(ExtFilter) || images_end < h.off_images || (h.off_tiles & 15) != 0 ||
        tiles_end > h.bytes) {
        set_error("%s: the plan's header is damaged", who);
        return MDC_EINVAL;
    }
    if (h.format != format) { set_error("%s: format is %d, the plan was made for %d", who, format, h.format); return MDC_EINVAL; }
    if (h.pairs_in != pairs_in) { set_error("%s: pairs_in is %lld, the plan was made for %lld", who, (long long)pairs_in, (long long)h.pairs_in); return MDC_EINVAL; }
    if (h.out_pairs != out_pairs) { set_error("%s: out_pairs is %lld, the plan was made for %lld", who, (long long)out_pairs, (long long)h.out_pairs); return MDC_EINVAL; }
    if ((rc = iq_pair_aligned(who, "input", format, iq_dev)) != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "output", out_dev, 4)) != MDC_OK) return rc;
    if ((rc = iq_aligned(who, "plan_dev", plan_dev, 8)) != MDC_OK) return rc;
    if (h.ntiles == 0) return MDC_OK;
    if (!iq_dev || !out_dev || !plan_dev) { set_error("%s: null buffer", who); return MDC_EINVAL; }
    const unsigned char* p = static_cast<const unsigned char*>(iq_dev);
    const unsigned char* pd = static_cast<const unsigned char*>(plan_dev);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    return guarded(who, [&]() -> int { return with_format(format, [&](auto fmt) { return extract_launch<decltype(fmt)::value>(p, pd, h, out_dev, s); }); });
}
