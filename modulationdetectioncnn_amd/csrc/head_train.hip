// Head training (include/mdc.h, "head training"): the dense layers of VT-CNN2 -- features K -> Dense(H, relu) -> Dense(C) ->
// softmax -- on feature rows that mdc_forward(..., MDC_TAP_FLAT) produced, in f32, with the conv layers frozen.  K is a multiple
// of 32 in 32..16384, H a multiple of 32 in 32..256, C in 2..16; VT-CNN2 is (10560, 256, C).
//
// One training batch = FIVE launches on the caller's stream, and a one-thread sixth that bumps Adam's step count when the update is
// applied (an evaluation: launches 1, 2 and 5), nothing allocated, no host synchronisation; every sum is taken in an order that depends on (count, K, H) only:
//   1 head_z1_kernel     Z1 = (F * s0) W1 on v_mfma_f32_32x32x2_f32.  Work-group = 128 batch rows x BN hidden units x one slice of
//                        K (4 waves, each 32 rows x BN; BN = the largest of 128 / 64 / 32 that divides H), feature rows gathered
//                        through `order`, the feature Dropout applied while the tile is staged.  The batch of 1,024 is only 16
//                        such tiles, so K is cut into S slices (about 512 work-groups in all) and each writes its partial sums.
//   2 head_row_kernel    one wave per row: z1 = the S partials in order + b1, ReLU, hidden Dropout, dense2, softmax, Keras'
//                        cross-entropy, dz2, dh = dz2 W2^T, dz1; writes h, dz1, dz2, the row's loss (evaluation: its hit flag).
//   3 head_dw1_kernel    dW1 = (F * s0)^T dZ1, the same MFMA with the feature index on the rows: work-group = 128 features x BN
//                        hidden units x one slice of the batch (S2 = 1..4 slices, about 512 work-groups), partial sums per slice.
//   4 head_small_kernel  dW2 = h^T dz2, db1, db2: one thread per hidden unit, up to 256 slices of the batch.
//   5 head_adam_kernel   sums the partials of 3 and 4 in order, divides by count, stores the gradient and applies TensorFlow
//                        2.4's Adam (train.hip's statement of it); its first work-group adds up the rows' losses.
//   6 head_step_kernel   apply != 0: iterations += 1, after launch 5 has read it everywhere.
// Stores are vector stores; no work-group waits for another or signals one; every register array is indexed by unrolled constants.
#include "train_common.h"
#include "train_host.h"             // the parameter bank and the entry bodies shared with train.hip

#include <cmath>
#include <cstddef>
#include <new>

struct mdc_head_trainer : mdc::ParamBank {      // two layers: (W1, b1), (W2, b2); d_state: HeadState
    int K = 0, H = 0, C = 0, BN = 32;
    int64_t max_batch = 0;
    int dw1_slices = 0;          // partial dW1 tensors d_dw1part holds
    size_t z1_floats = 0;        // floats d_z1part holds
    float rate0 = 0.f, rate1 = 0.f;
    unsigned drop_seed = 0;
    float *d_z1part = nullptr, *d_dw1part = nullptr, *d_small = nullptr;      // partial sums of launches 1, 3 and 4
    float *d_h = nullptr, *d_dz1 = nullptr, *d_dz2 = nullptr, *d_loss = nullptr;      // per batch position
    int* d_hit = nullptr;
};

namespace mdc {

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kHeadBM = 128, kHeadBK = 32;      // rows (launch 1) / features (launch 3) per work-group; depth of one staged tile
constexpr int kHeadLda = kHeadBM + 2;           // launch 1 stages its feature tile transposed ([k][row]): 130 spreads the 4 x 8 stores of a wave over all banks
constexpr int kHeadTarget = 512;                // work-groups launch 1 aims for when it slices K
constexpr int kHeadCmax = 16, kHeadHmax = 256;
constexpr int kHeadMaxSlices2 = 4;               // partial dW1 tensors launch 3 may write (each K x H floats)
constexpr int kSmallSlices = 256, kSmallRows = 16, kSmallStride = kHeadHmax * kHeadCmax + kHeadHmax + kHeadCmax;      // launch 4: slices of >= 16 rows; a partial = dW2 [h][16], db1 [h], db2 [16]

struct HeadState {
    long long iterations;      // Adam's step count
    long long train_rows;
    double train_loss;
    long long eval_rows;
    double eval_loss;
    long long eval_correct;
    unsigned bad_indices;      // batch positions skipped because their index lay outside [0, n_rows)
};
static_assert(offsetof(HeadState, iterations) == 0, "bank_set_iterations writes the record's first field");

struct HeadPlan { int tiles_m, slices, chunks_per, slices2, rows_per2, small; };

HeadPlan head_plan(int K, int H, int BN, int64_t count) {
    HeadPlan p;
    p.tiles_m = (int)((count + kHeadBM - 1) / kHeadBM);
    const int tiles = p.tiles_m * (H / BN), chunks = K / kHeadBK;
    int s = kHeadTarget / tiles;
    s = s < 1 ? 1 : (s > chunks ? chunks : s);
    p.chunks_per = (chunks + s - 1) / s;
    p.slices = (chunks + p.chunks_per - 1) / p.chunks_per;
    // launch 3 has ceil(K / 128) x H / BN tiles (VT-CNN2: 166): up to four slices of the batch, each at least one 32-row stage
    const int64_t stages = (count + kHeadBK - 1) / kHeadBK;
    int64_t s2 = kHeadTarget / (((K + kHeadBM - 1) / kHeadBM) * (H / BN));
    s2 = s2 > kHeadMaxSlices2 ? kHeadMaxSlices2 : s2;
    s2 = s2 > stages ? stages : s2;
    s2 = s2 < 1 ? 1 : s2;
    p.rows_per2 = (int)((stages + s2 - 1) / s2 * kHeadBK);
    p.slices2 = (int)((count + p.rows_per2 - 1) / p.rows_per2);
    p.small = (int)((count + kSmallRows - 1) / kSmallRows);
    if (p.small > kSmallSlices) p.small = kSmallSlices;
    return p;
}

__device__ __forceinline__ float4 drop4(float4 v, unsigned key, unsigned e0, const DropArgs& d) {
    v.x = drop_keep(key, e0, d.thr) ? v.x * d.inv : 0.f;
    v.y = drop_keep(key, e0 + 1u, d.thr) ? v.y * d.inv : 0.f;
    v.z = drop_keep(key, e0 + 2u, d.thr) ? v.z * d.inv : 0.f;
    v.w = drop_keep(key, e0 + 3u, d.thr) ? v.w * d.inv : 0.f;
    return v;
}

// ---- launch 1: partial Z1.  grid (row tiles, H / BN, K slices); part[slice][tiles_m * 128][H]
template <int BN, bool DROP>
__global__ __launch_bounds__(256) void head_z1_kernel(const float* __restrict__ feat, long n_rows, const int* __restrict__ order, long first, int count,
                                                     int K, int H, const float* __restrict__ W1, float* __restrict__ part, int chunks_per,
                                                     HeadState* __restrict__ st, DropArgs drop) {
    constexpr int NT = BN / 32;
    __shared__ float sA[kHeadBK * kHeadLda];                               // [k][row]
    __shared__ __attribute__((aligned(16))) float sB[kHeadBK * BN];        // [k][hidden unit]
    __shared__ long sIdx[kHeadBM];
    __shared__ unsigned sKey[kHeadBM];
    const int t = threadIdx.x, w = t >> 6, lane = t & 63, half = lane >> 5, r = lane & 31;
    const int m0 = blockIdx.x * kHeadBM, n0 = blockIdx.y * BN;
    const int c_lo = blockIdx.z * chunks_per, c_hi = min(K / kHeadBK, c_lo + chunks_per);
    if (t < kHeadBM) {
        const long idx = m0 + t < count ? frame_index(order, first, m0 + t, n_rows, st, blockIdx.y == 0 && blockIdx.z == 0) : -1;
        sIdx[t] = idx;
        sKey[t] = DROP && idx >= 0 ? drop_frame_key(drop_step_key(drop, st), idx, 0u) : 0u;
    }
    __syncthreads();
    float4 ra[4], rb[NT];
    auto fetch = [&](int c) {
        const int k0 = c * kHeadBK;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int id = t + 256 * i, row = id >> 3, kq = id & 7;
            const long idx = sIdx[row];
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (idx >= 0) v = *reinterpret_cast<const float4*>(feat + idx * K + k0 + 4 * kq);
            if (DROP) v = drop4(v, sKey[row], (unsigned)(k0 + 4 * kq), drop);
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int id = t + 256 * i, kr = id / (BN / 4), q = id % (BN / 4);
            const float4 v = *reinterpret_cast<const float4*>(W1 + (size_t)(k0 + kr) * H + n0 + 4 * q);
            rb[i] = v;
        }
    };
    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[nt][e] = 0.f;
    fetch(c_lo);
    for (int c = c_lo; c < c_hi; ++c) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int id = t + 256 * i, row = id >> 3, kq = id & 7;
            sA[(4 * kq + 0) * kHeadLda + row] = ra[i].x;
            sA[(4 * kq + 1) * kHeadLda + row] = ra[i].y;
            sA[(4 * kq + 2) * kHeadLda + row] = ra[i].z;
            sA[(4 * kq + 3) * kHeadLda + row] = ra[i].w;
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int id = t + 256 * i, kr = id / (BN / 4), q = id % (BN / 4);
            const float4 v = rb[i];
            *reinterpret_cast<float4*>(sB + kr * BN + 4 * q) = v;
        }
        __syncthreads();
        if (c + 1 < c_hi) fetch(c + 1);      // the next tile's loads fly under this tile's MFMAs
#pragma unroll
        for (int kk = 0; kk < kHeadBK / 2; ++kk) {
            const float a = sA[(2 * kk + half) * kHeadLda + 32 * w + r];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, sB[(2 * kk + half) * BN + 32 * nt + r], acc[nt], 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D layout: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5); rows past `count` land in the padded tile
    float* out = part + ((size_t)blockIdx.z * gridDim.x * kHeadBM + m0 + 32 * w) * H + n0 + r;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int e = 0; e < 16; ++e) out[(size_t)((e & 3) + 8 * (e >> 2) + 4 * half) * H + 32 * nt] = acc[nt][e];
}

// ---- launch 2: the rest of the forward, the loss and the small backward products, one wave per row
template <bool TRAIN, bool DROP>
__global__ __launch_bounds__(256) void head_row_kernel(const float* __restrict__ y, long n_rows, const int* __restrict__ order, long first, int count,
                                                      int H, int C, const float* __restrict__ part, int slices, size_t slice_stride,
                                                      const float* __restrict__ b1, const float* __restrict__ W2, const float* __restrict__ b2,
                                                      float* __restrict__ hbuf, float* __restrict__ dz1buf, float* __restrict__ dz2buf,
                                                      float* __restrict__ lossrow, int* __restrict__ hit, HeadState* __restrict__ st, DropArgs drop) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
    float w2[4][kHeadCmax], b1v[4], b2v[kHeadCmax];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int hh = lane + 64 * j;
        b1v[j] = hh < H ? b1[hh] : 0.f;
#pragma unroll
        for (int c = 0; c < kHeadCmax; ++c) w2[j][c] = (hh < H && c < C) ? W2[hh * C + c] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < kHeadCmax; ++c) b2v[c] = c < C ? b2[c] : 0.f;
    const unsigned kstep = DROP ? drop_step_key(drop, st) : 0u;
    for (int pos = wave; pos < count; pos += nwaves) {
        const long idx = frame_index(order, first, pos, n_rows, st, false);      // (counted by launch 1)
        const unsigned key = DROP && idx >= 0 ? drop_frame_key(kstep, idx, 1u) : 0u;
        float z1[4], hv[4], m1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int hh = lane + 64 * j;
            float s = 0.f;
            if (hh < H) {      // the slices in order; eight loads in flight at a time (one dependent load per addition is 30 round trips)
                const float* src = part + (size_t)pos * H + hh;
                int sl = 0;
                for (; sl + 8 <= slices; sl += 8, src += 8 * slice_stride) {
                    float t8[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) t8[u] = src[(size_t)u * slice_stride];
#pragma unroll
                    for (int u = 0; u < 8; ++u) s += t8[u];
                }
                for (; sl < slices; ++sl, src += slice_stride) s += *src;
            }
            z1[j] = s + b1v[j];
            m1[j] = DROP && idx >= 0 ? (drop_keep(key, (unsigned)hh, drop.thr) ? drop.inv : 0.f) : 1.f;
            hv[j] = hh < H ? fmaxf(z1[j], 0.f) * m1[j] : 0.f;
        }
        float z2[kHeadCmax], yv[kHeadCmax];
#pragma unroll
        for (int c = 0; c < kHeadCmax; ++c) {
            const float s = (hv[0] * w2[0][c] + hv[1] * w2[1][c]) + (hv[2] * w2[2][c] + hv[3] * w2[3][c]);
            z2[c] = wave_allsum(s) + b2v[c];
            yv[c] = (idx >= 0 && c < C) ? y[idx * C + c] : 0.f;
        }
        // softmax, Keras' categorical cross-entropy on the probabilities, d loss / d z2 (train.hip's softmax_xent, keeping p)
        float mx = z2[0];
#pragma unroll
        for (int c = 1; c < kHeadCmax; ++c) if (c < C) mx = fmaxf(mx, z2[c]);
        float p[kHeadCmax], se = 0.f;
#pragma unroll
        for (int c = 0; c < kHeadCmax; ++c) { p[c] = c < C ? expf(z2[c] - mx) : 0.f; se += p[c]; }
        float sp = 0.f;
#pragma unroll
        for (int c = 0; c < kHeadCmax; ++c) { p[c] = p[c] / se; sp += p[c]; }
        float li = 0.f, sg = 0.f, gq[kHeadCmax], q[kHeadCmax];
#pragma unroll
        for (int c = 0; c < kHeadCmax; ++c) {
            q[c] = p[c] / sp;
            const float qc = fminf(fmaxf(q[c], kKerasEps), 1.f - kKerasEps);
            const bool in = c < C && q[c] >= kKerasEps && q[c] <= 1.f - kKerasEps;
            if (c < C && yv[c] != 0.f) li -= yv[c] * logf(qc);
            gq[c] = in ? -yv[c] / qc : 0.f;
            sg += gq[c] * q[c];
        }
        if (lane == 0) lossrow[pos] = li;
        if (!TRAIN) {
            // arg-max of p against arg-max of the target row, the lowest index on a tie on both sides
            int ap = 0, ay = 0;
            float bp = p[0], by = yv[0];
#pragma unroll
            for (int c = 1; c < kHeadCmax; ++c) {
                if (c < C && p[c] > bp) { bp = p[c]; ap = c; }
                if (c < C && yv[c] > by) { by = yv[c]; ay = c; }
            }
            if (lane == 0) hit[pos] = (idx >= 0 && ap == ay) ? 1 : 0;
            continue;
        }
        float spg = 0.f, gp[kHeadCmax], gz[kHeadCmax];
#pragma unroll
        for (int c = 0; c < kHeadCmax; ++c) { gp[c] = (gq[c] - sg) / sp; spg += gp[c] * p[c]; }
        float mine = 0.f;      // lane c < 16 stores dz2[c] (zero past C)
#pragma unroll
        for (int c = 0; c < kHeadCmax; ++c) {
            gz[c] = p[c] * (gp[c] - spg);
            mine = lane == c ? gz[c] : mine;
        }
        if (lane < kHeadCmax) dz2buf[(size_t)pos * kHeadCmax + lane] = mine;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int hh = lane + 64 * j;
            float dh = 0.f;
#pragma unroll
            for (int c = 0; c < kHeadCmax; ++c) dh = fmaf(gz[c], w2[j][c], dh);
            if (hh < H) {
                hbuf[(size_t)pos * H + hh] = hv[j];
                dz1buf[(size_t)pos * H + hh] = z1[j] > 0.f ? dh * m1[j] : 0.f;
            }
        }
    }
}

// ---- launch 3: partial dW1.  grid (ceil(K / 128), H / BN, batch slices); part[slice][K][H]
template <int BN, bool DROP>
__global__ __launch_bounds__(256) void head_dw1_kernel(const float* __restrict__ feat, long n_rows, const int* __restrict__ order, long first, int count,
                                                      int K, int H, const float* __restrict__ dz1buf, float* __restrict__ part, int rows_per,
                                                      HeadState* __restrict__ st, DropArgs drop) {
    constexpr int NT = BN / 32;
    __shared__ __attribute__((aligned(16))) float sA[kHeadBK * kHeadBM];      // [row][feature]
    __shared__ __attribute__((aligned(16))) float sB[kHeadBK * BN];           // [row][hidden unit]
    const int t = threadIdx.x, w = t >> 6, lane = t & 63, half = lane >> 5, r = lane & 31;
    const int k0 = blockIdx.x * kHeadBM, n0 = blockIdx.y * BN;
    const int r_lo = blockIdx.z * rows_per, r_hi = min(count, r_lo + rows_per);
    const unsigned kstep = DROP ? drop_step_key(drop, st) : 0u;
    float4 ra[4], rb[NT];
    long nidx[4];      // the rows of the NEXT fetch: their indices are read one stage ahead, so that no fetch waits for `order`
    auto fetch_idx = [&](int r0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = (t + 256 * i) >> 5;
            nidx[i] = r0 + row < r_hi ? frame_index(order, first, r0 + row, n_rows, st, false) : -1;
        }
    };
    auto fetch = [&](int r0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int kq = (t + 256 * i) & 31, k = k0 + 4 * kq;
            const long idx = nidx[i];
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (idx >= 0 && k < K) v = *reinterpret_cast<const float4*>(feat + idx * K + k);
            if (DROP && idx >= 0) v = drop4(v, drop_frame_key(kstep, idx, 0u), (unsigned)k, drop);
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int id = t + 256 * i, row = id / (BN / 4), q = id % (BN / 4);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r0 + row < r_hi) v = *reinterpret_cast<const float4*>(dz1buf + (size_t)(r0 + row) * H + n0 + 4 * q);
            rb[i] = v;
        }
        fetch_idx(r0 + kHeadBK);
    };
    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[nt][e] = 0.f;
    fetch_idx(r_lo);
    fetch(r_lo);
    for (int r0 = r_lo; r0 < r_hi; r0 += kHeadBK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int id = t + 256 * i;
            const float4 v = ra[i];
            *reinterpret_cast<float4*>(sA + (id >> 5) * kHeadBM + 4 * (id & 31)) = v;
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int id = t + 256 * i;
            const float4 v = rb[i];
            *reinterpret_cast<float4*>(sB + (id / (BN / 4)) * BN + 4 * (id % (BN / 4))) = v;
        }
        __syncthreads();
        if (r0 + kHeadBK < r_hi) fetch(r0 + kHeadBK);
#pragma unroll
        for (int kk = 0; kk < kHeadBK / 2; ++kk) {
            const float a = sA[(2 * kk + half) * kHeadBM + 32 * w + r];      // A[feature][batch row]
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, sB[(2 * kk + half) * BN + 32 * nt + r], acc[nt], 0, 0, 0);
        }
        __syncthreads();
    }
    if (k0 + 32 * w >= K) return;      // K is a multiple of 32: a wave's 32 features are all there or all past the end
    float* out = part + ((size_t)blockIdx.z * K + k0 + 32 * w) * H + n0 + r;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int e = 0; e < 16; ++e) out[(size_t)((e & 3) + 8 * (e >> 2) + 4 * half) * H + 32 * nt] = acc[nt][e];
}

// ---- launch 4: dW2 = h^T dz2, db1 = sum dz1, db2 = sum dz2 over one slice of the batch; thread = hidden unit
__global__ __launch_bounds__(256) void head_small_kernel(const float* __restrict__ hbuf, const float* __restrict__ dz1buf, const float* __restrict__ dz2buf,
                                                        int count, int H, float* __restrict__ small) {
    const int t = threadIdx.x;
    const int per = (count + gridDim.x - 1) / gridDim.x, lo = blockIdx.x * per, hi = min(count, lo + per);
    float g2[kHeadCmax], g1 = 0.f, gb2 = 0.f;
#pragma unroll
    for (int c = 0; c < kHeadCmax; ++c) g2[c] = 0.f;
#pragma unroll 4
    for (int pos = lo; pos < hi; ++pos) {
        const float4* d4 = reinterpret_cast<const float4*>(dz2buf + (size_t)pos * kHeadCmax);
        const float4 d0 = d4[0], d1 = d4[1], d2 = d4[2], d3 = d4[3];
        const float dz[kHeadCmax] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w, d2.x, d2.y, d2.z, d2.w, d3.x, d3.y, d3.z, d3.w};
        const float hv = t < H ? hbuf[(size_t)pos * H + t] : 0.f;
        if (t < H) g1 += dz1buf[(size_t)pos * H + t];
        if (t < kHeadCmax) gb2 += dz2buf[(size_t)pos * kHeadCmax + t];
#pragma unroll
        for (int c = 0; c < kHeadCmax; ++c) g2[c] = fmaf(hv, dz[c], g2[c]);
    }
    float* out = small + (size_t)blockIdx.x * kSmallStride;
    float4* o4 = reinterpret_cast<float4*>(out + t * kHeadCmax);
    o4[0] = make_float4(g2[0], g2[1], g2[2], g2[3]);
    o4[1] = make_float4(g2[4], g2[5], g2[6], g2[7]);
    o4[2] = make_float4(g2[8], g2[9], g2[10], g2[11]);
    o4[3] = make_float4(g2[12], g2[13], g2[14], g2[15]);
    out[kHeadHmax * kHeadCmax + t] = g1;
    if (t < kHeadCmax) out[kHeadHmax * kHeadCmax + kHeadHmax + t] = gb2;
}

// ---- launch 5: fixed-order sums of the partials, the gradient of the MEAN loss, TensorFlow 2.4's Adam; the batch's statistics.
// mode: 0 = statistics of an evaluation (one work-group), 1 = gradient stored, 2 = gradient stored and applied.
// Work-groups 0 .. w1_blocks - 1 take W1 four parameters per thread, the rest b1, W2 and b2 one per thread.
__global__ __launch_bounds__(256) void head_adam_kernel(const float* __restrict__ dw1part, int slices2, const float* __restrict__ small, int nsmall,
                                                       int K, int H, int C, int count, int mode, int w1_blocks, float lr, float beta1, float beta2, float eps,
                                                       float* __restrict__ params, float* __restrict__ m, float* __restrict__ v, float* __restrict__ grad,
                                                       const float* __restrict__ lossrow, const int* __restrict__ hit, HeadState* __restrict__ st) {
    __shared__ double lpart[256];
    __shared__ int hpart[256];
    __shared__ float s_alpha;
    const size_t nW1 = (size_t)K * H, nvec = nW1 / 4, ntail = (size_t)H + (size_t)H * C + C;
    if (threadIdx.x == 0) s_alpha = mode == 2 ? adam_alpha(lr, beta1, beta2, st->iterations + 1) : 0.f;      // `iterations` is bumped by launch 6
    __syncthreads();
    const float alpha = s_alpha, inv_n = 1.f / (float)count;
    if (mode != 0 && (int)blockIdx.x < w1_blocks) {
        const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
        if (q < nvec) {
            float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int s = 0; s < slices2; ++s) {
                const float4 d = reinterpret_cast<const float4*>(dw1part)[(size_t)s * nvec + q];
                g.x += d.x; g.y += d.y; g.z += d.z; g.w += d.w;
            }
            g.x *= inv_n; g.y *= inv_n; g.z *= inv_n; g.w *= inv_n;
            reinterpret_cast<float4*>(grad)[q] = g;
            if (mode == 2) {
                float4 mi = reinterpret_cast<float4*>(m)[q], vi = reinterpret_cast<float4*>(v)[q], wi = reinterpret_cast<float4*>(params)[q];
                adam_update(g.x, mi.x, vi.x, wi.x, alpha, beta1, beta2, eps);
                adam_update(g.y, mi.y, vi.y, wi.y, alpha, beta1, beta2, eps);
                adam_update(g.z, mi.z, vi.z, wi.z, alpha, beta1, beta2, eps);
                adam_update(g.w, mi.w, vi.w, wi.w, alpha, beta1, beta2, eps);
                reinterpret_cast<float4*>(m)[q] = mi;
                reinterpret_cast<float4*>(v)[q] = vi;
                reinterpret_cast<float4*>(params)[q] = wi;
            }
        }
    } else if (mode != 0) {
        const size_t j = (size_t)((int)blockIdx.x - w1_blocks) * 256 + threadIdx.x;
        if (j < ntail) {
            size_t e;      // the entry of a launch-4 partial that is this parameter
            if (j < (size_t)H) e = (size_t)kHeadHmax * kHeadCmax + j;                                       // b1
            else if (j < (size_t)H + (size_t)H * C) { const size_t u = j - H; e = (u / C) * kHeadCmax + u % C; }      // W2[h][c]
            else e = (size_t)kHeadHmax * kHeadCmax + kHeadHmax + (j - H - (size_t)H * C);                   // b2
            float gsum = 0.f;
            for (int s = 0; s < nsmall; ++s) gsum += small[(size_t)s * kSmallStride + e];
            const float gmean = gsum * inv_n;
            const size_t i = nW1 + j;
            grad[i] = gmean;
            if (mode == 2) {
                float mi = m[i], vi = v[i], wi = params[i];
                adam_update(gmean, mi, vi, wi, alpha, beta1, beta2, eps);
                m[i] = mi; v[i] = vi; params[i] = wi;
            }
        }
    }
    if (blockIdx.x == 0) {      // the batch's summed loss (and hits): each thread its rows in order, then a fixed tree
        double l = 0.0;
        int hsum = 0;
        for (int pos = threadIdx.x; pos < count; pos += 256) {
            l += (double)lossrow[pos];
            if (mode == 0) hsum += hit[pos];
        }
        lpart[threadIdx.x] = l;
        hpart[threadIdx.x] = hsum;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) { lpart[threadIdx.x] += lpart[threadIdx.x + s]; hpart[threadIdx.x] += hpart[threadIdx.x + s]; }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            if (mode == 0) { st->eval_loss += lpart[0]; st->eval_rows += count; st->eval_correct += hpart[0]; }
            else { st->train_loss += lpart[0]; st->train_rows += count; }
        }
    }
}

// ---- launch 6 (apply != 0 only): Adam's step count advances once the whole of launch 5 has read it.  A launch of its own, not a
// ticket taken by launch 5's work-groups: the release fence in front of such a ticket writes the L2's dirty lines back, and 2,653
// work-groups doing that behind 32 MB of fresh moments and weights cost 100 us (measured; train.hip's 37 work-groups do not notice).
__global__ void head_step_kernel(HeadState* __restrict__ st) {
    if (threadIdx.x == 0) st->iterations += 1;
}

DropArgs drop_args(unsigned seed, float rate) {
    return DropArgs{seed, (unsigned)std::floor((double)rate * 4294967296.0), 1.f / (1.f - rate)};
}

template <int BN>
int head_launch_bn(mdc_head_trainer* t, const float* f, const float* y, int64_t n_rows, const int32_t* order, int64_t first, int cnt, int mode, hipStream_t s) {
    auto* st = static_cast<HeadState*>(t->d_state);
    const int K = t->K, H = t->H, C = t->C;
    const HeadPlan p = head_plan(K, H, BN, cnt);
    if (p.slices2 > t->dw1_slices || (size_t)p.slices * p.tiles_m * kHeadBM * H > t->z1_floats) {      // never: the bounds of mdc_head_trainer_create
        set_error("head training: the plan of %d rows (%d x %d slices) exceeds the scratch allocated for max_batch %lld", cnt, p.slices, p.slices2,
                  (long long)t->max_batch);
        return MDC_EIO;
    }
    // Dropout acts in training batches only (Keras' fit reports the loss WITH it and evaluates val_loss without)
    const bool d0 = mode != 0 && t->rate0 > 0.f, d1 = mode != 0 && t->rate1 > 0.f;
    const DropArgs a0 = drop_args(t->drop_seed, t->rate0), a1 = drop_args(t->drop_seed, t->rate1);
    float *W1 = t->d_params + t->off_k[0], *b1 = t->d_params + t->off_b[0], *W2 = t->d_params + t->off_k[1], *b2 = t->d_params + t->off_b[1];
    const dim3 g1(p.tiles_m, H / BN, p.slices);
    if (d0) hipLaunchKernelGGL((head_z1_kernel<BN, true>), g1, dim3(256), 0, s, f, (long)n_rows, order, (long)first, cnt, K, H, W1, t->d_z1part, p.chunks_per, st, a0);
    else hipLaunchKernelGGL((head_z1_kernel<BN, false>), g1, dim3(256), 0, s, f, (long)n_rows, order, (long)first, cnt, K, H, W1, t->d_z1part, p.chunks_per, st, a0);
    MDC_HIP(hipGetLastError());
    const int gr = (cnt + 3) / 4 < 1024 ? (cnt + 3) / 4 : 1024;
    const size_t stride = (size_t)p.tiles_m * kHeadBM * H;
#define MDC_HEAD_ROW(TR, DR) hipLaunchKernelGGL((head_row_kernel<TR, DR>), dim3(gr), dim3(256), 0, s, y, (long)n_rows, order, (long)first, cnt, H, C, t->d_z1part, p.slices, \
                                                 stride, b1, W2, b2, t->d_h, t->d_dz1, t->d_dz2, t->d_loss, t->d_hit, st, a1)
    if (mode == 0) MDC_HEAD_ROW(false, false);
    else if (d1) MDC_HEAD_ROW(true, true);
    else MDC_HEAD_ROW(true, false);
#undef MDC_HEAD_ROW
    MDC_HIP(hipGetLastError());
    if (mode != 0) {
        const dim3 g3((K + kHeadBM - 1) / kHeadBM, H / BN, p.slices2);
        if (d0) hipLaunchKernelGGL((head_dw1_kernel<BN, true>), g3, dim3(256), 0, s, f, (long)n_rows, order, (long)first, cnt, K, H, t->d_dz1, t->d_dw1part, p.rows_per2, st, a0);
        else hipLaunchKernelGGL((head_dw1_kernel<BN, false>), g3, dim3(256), 0, s, f, (long)n_rows, order, (long)first, cnt, K, H, t->d_dz1, t->d_dw1part, p.rows_per2, st, a0);
        MDC_HIP(hipGetLastError());
        hipLaunchKernelGGL(head_small_kernel, dim3(p.small), dim3(256), 0, s, t->d_h, t->d_dz1, t->d_dz2, cnt, H, t->d_small);
        MDC_HIP(hipGetLastError());
    }
    const int w1_blocks = (int)((t->nk[0] / 4 + 255) / 256), tail_blocks = (int)((t->P - t->nk[0] + 255) / 256);
    const int blocks = mode == 0 ? 1 : w1_blocks + tail_blocks;
    hipLaunchKernelGGL(head_adam_kernel, dim3(blocks), dim3(256), 0, s, t->d_dw1part, p.slices2, t->d_small, p.small, K, H, C, cnt, mode, w1_blocks, t->lr, t->beta1, t->beta2, t->eps,
                       t->d_params, t->d_m, t->d_v, t->d_grad, t->d_loss, t->d_hit, st);
    MDC_HIP(hipGetLastError());
    if (mode == 2) {
        hipLaunchKernelGGL(head_step_kernel, dim3(1), dim3(64), 0, s, st);
        MDC_HIP(hipGetLastError());
    }
    return MDC_OK;
}

int head_launch(mdc_head_trainer* t, const float* f, const float* y, int64_t n_rows, const int32_t* order, int64_t first, int64_t count, int mode, hipStream_t s) {
    if (t->BN == 128) return head_launch_bn<128>(t, f, y, n_rows, order, first, (int)count, mode, s);
    if (t->BN == 64) return head_launch_bn<64>(t, f, y, n_rows, order, first, (int)count, mode, s);
    return head_launch_bn<32>(t, f, y, n_rows, order, first, (int)count, mode, s);
}

// mdc_head_train_batch (mode 1: gradient only, 2: gradient + Adam) and mdc_head_trainer_evaluate (mode 0) behind their names
int batch_entry(const char* who, mdc_head_trainer* t, const float* f, const float* y, int64_t n_rows, const int32_t* order, int64_t first, int64_t count,
                int mode, void* hip_stream) {
    return guarded(who, [&]() -> int {
        int rc = bank_check_batch(who, t, "features", "rows", f, y, n_rows, order, first, count);
        if (rc != MDC_OK) return rc;
        // the head's own bounds: all scratch was allocated for max_batch rows
        if (count > t->max_batch) { set_error("%s: count %lld exceeds the trainer's max_batch %lld", who, (long long)count, (long long)t->max_batch); return MDC_EINVAL; }
        if (first > ((int64_t)1 << 40)) { set_error("%s: first out of range", who); return MDC_EINVAL; }
        if (count == 0) return MDC_OK;
        DeviceScope dev(t->device);
        if (!device_selected(who, dev)) return MDC_EIO;
        return head_launch(t, f, y, n_rows, order, first, count, mode, static_cast<hipStream_t>(hip_stream));
    });
}

}  // namespace

}  // namespace mdc

using namespace mdc;

extern "C" {

int mdc_head_trainer_create(int features, int hidden, int classes, int64_t max_batch, int device, mdc_head_trainer** out) {
    return guarded("mdc_head_trainer_create", [&]() -> int {
        if (!out) { set_error("mdc_head_trainer_create: null argument"); return MDC_EINVAL; }
        *out = nullptr;
        if (features < 32 || features > 16384 || features % 32 != 0) { set_error("mdc_head_trainer_create: features must be a multiple of 32 in 32..16384 (got %d)", features); return MDC_EINVAL; }
        if (hidden < 32 || hidden > kHeadHmax || hidden % 32 != 0) { set_error("mdc_head_trainer_create: hidden must be a multiple of 32 in 32..256 (got %d)", hidden); return MDC_EINVAL; }
        if (classes < 2 || classes > kHeadCmax) { set_error("mdc_head_trainer_create: classes must lie in 2..16 (got %d)", classes); return MDC_EINVAL; }
        if (max_batch < 1 || max_batch > 65536) { set_error("mdc_head_trainer_create: max_batch must lie in 1..65536 (got %lld)", (long long)max_batch); return MDC_EINVAL; }
        int rc = check_device(device);      // (behind the argument checks: a bad shape is MDC_EINVAL on a machine without a GPU too)
        if (rc != MDC_OK) return rc;
        mdc_head_trainer* t = new (std::nothrow) mdc_head_trainer();
        if (!t) { set_error("out of host memory"); return MDC_ENOMEM; }
        t->K = features; t->H = hidden; t->C = classes; t->max_batch = max_batch; t->device = device;
        t->BN = hidden % 128 == 0 ? 128 : (hidden % 64 == 0 ? 64 : 32);
        t->nlayers = 2;
        t->nk[0] = (size_t)features * hidden;  t->nb[0] = hidden;
        t->nk[1] = (size_t)hidden * classes;   t->nb[1] = classes;
        t->layout();
        DeviceScope dev(device);
        if (!device_selected("mdc_head_trainer_create", dev)) { delete t; return MDC_EIO; }
        // scratch for the largest batch: launch 1 writes slices x tiles x (128 x BN) floats, and head_plan keeps slices x tiles at or
        // under max(kHeadTarget, tiles).  Launch 3 writes slices2 partial dW1, and slices2 is NOT monotone in count (96 rows are
        // three one-stage slices, 128 rows two two-stage ones): its bound over every count <= max_batch is the cap or the stages
        // of max_batch, whichever is smaller.  head_launch_bn checks both plans against what was allocated.
        const HeadPlan pm = head_plan(features, hidden, t->BN, max_batch);
        const int64_t stages_max = (max_batch + kHeadBK - 1) / kHeadBK;
        t->dw1_slices = (int)(stages_max < kHeadMaxSlices2 ? stages_max : kHeadMaxSlices2);
        const size_t tiles = (size_t)pm.tiles_m * (hidden / t->BN);
        const size_t z1f = (tiles > (size_t)kHeadTarget ? tiles : (size_t)kHeadTarget) * kHeadBM * t->BN;
        t->z1_floats = z1f;
        const size_t mb = (size_t)max_batch;
        auto fail = [&](int code) { mdc_head_trainer_destroy(t); return code; };
        rc = t->alloc("mdc_head_trainer_create", sizeof(HeadState));
        if (rc != MDC_OK) return fail(rc);
        if (hipMalloc(&t->d_z1part, z1f * sizeof(float)) != hipSuccess ||
            hipMalloc(&t->d_dw1part, (size_t)t->dw1_slices * t->nk[0] * sizeof(float)) != hipSuccess ||
            hipMalloc(&t->d_small, (size_t)kSmallSlices * kSmallStride * sizeof(float)) != hipSuccess ||
            hipMalloc(&t->d_h, mb * hidden * sizeof(float)) != hipSuccess || hipMalloc(&t->d_dz1, mb * hidden * sizeof(float)) != hipSuccess ||
            hipMalloc(&t->d_dz2, mb * kHeadCmax * sizeof(float)) != hipSuccess || hipMalloc(&t->d_loss, mb * sizeof(float)) != hipSuccess ||
            hipMalloc(&t->d_hit, mb * sizeof(int)) != hipSuccess) {
            set_error("mdc_head_trainer_create: out of device memory");
            return fail(MDC_ENOMEM);
        }
        *out = t;
        return MDC_OK;
    });
}

int mdc_head_trainer_set_adam(mdc_head_trainer* t, float lr, float beta1, float beta2, float eps) {
    return bank_set_adam("mdc_head_trainer_set_adam", t, lr, beta1, beta2, eps);
}

int mdc_head_trainer_set_dropout(mdc_head_trainer* t, float rate_features, float rate_hidden, uint32_t seed) {
    if (!t) { set_error("null trainer"); return MDC_EINVAL; }
    if (!(rate_features >= 0.f && rate_features < 1.f) || !(rate_hidden >= 0.f && rate_hidden < 1.f)) {
        set_error("mdc_head_trainer_set_dropout: need 0 <= rate < 1 for both rates");
        return MDC_EINVAL;
    }
    t->rate0 = rate_features; t->rate1 = rate_hidden; t->drop_seed = seed;
    return MDC_OK;
}

int mdc_head_trainer_set_tensor(mdc_head_trainer* t, int which, int layer, const float* kernel_host, size_t kernel_elems, const float* bias_host,
                                size_t bias_elems, void* hip_stream) {
    return guarded("mdc_head_trainer_set_tensor", [&]() -> int {
        return bank_set_tensor("mdc_head_trainer_set_tensor", t, which, layer, kernel_host, kernel_elems, bias_host, bias_elems, static_cast<hipStream_t>(hip_stream));
    });
}

int mdc_head_trainer_get_tensor(mdc_head_trainer* t, int which, int layer, float* kernel_host, size_t kernel_elems, float* bias_host, size_t bias_elems,
                                void* hip_stream) {
    return guarded("mdc_head_trainer_get_tensor", [&]() -> int {
        return bank_get_tensor("mdc_head_trainer_get_tensor", t, which, layer, kernel_host, kernel_elems, bias_host, bias_elems, static_cast<hipStream_t>(hip_stream));
    });
}

int mdc_head_trainer_set_iterations(mdc_head_trainer* t, int64_t iterations, void* hip_stream) {
    return guarded("mdc_head_trainer_set_iterations", [&]() -> int {
        return bank_set_iterations("mdc_head_trainer_set_iterations", t, iterations, static_cast<hipStream_t>(hip_stream));
    });
}

int mdc_head_train_batch(mdc_head_trainer* t, const float* feat_dev, const float* y_dev, int64_t n_rows, const int32_t* order_dev, int64_t first,
                         int64_t count, int apply, void* hip_stream) {
    return batch_entry("mdc_head_train_batch", t, feat_dev, y_dev, n_rows, order_dev, first, count, apply ? 2 : 1, hip_stream);
}

int mdc_head_trainer_evaluate(mdc_head_trainer* t, const float* feat_dev, const float* y_dev, int64_t n_rows, const int32_t* order_dev, int64_t first,
                              int64_t count, void* hip_stream) {
    return batch_entry("mdc_head_trainer_evaluate", t, feat_dev, y_dev, n_rows, order_dev, first, count, 0, hip_stream);
}

int mdc_head_trainer_read(mdc_head_trainer* t, int reset, double* train_loss_sum, int64_t* train_rows, double* eval_loss_sum, int64_t* eval_rows,
                          int64_t* eval_correct, int64_t* iterations, void* hip_stream) {
    return guarded("mdc_head_trainer_read", [&]() -> int {
        HeadState h{};
        int rc = bank_read_state("mdc_head_trainer_read", t, reset, &h, sizeof(h), offsetof(HeadState, train_rows), static_cast<hipStream_t>(hip_stream));
        if (rc != MDC_OK) return rc;
        if (train_loss_sum) *train_loss_sum = h.train_loss;
        if (train_rows) *train_rows = h.train_rows;
        if (eval_loss_sum) *eval_loss_sum = h.eval_loss;
        if (eval_rows) *eval_rows = h.eval_rows;
        if (eval_correct) *eval_correct = h.eval_correct;
        if (iterations) *iterations = h.iterations;
        if (h.bad_indices) {      // (the statistics above are those of the rows that WERE addressable)
            set_error("mdc_head_trainer_read: %u batch positions named rows outside [0, n_rows) -- skipped, not trained on; check order_dev", h.bad_indices);
            return MDC_EINVAL;
        }
        return MDC_OK;
    });
}

void mdc_head_trainer_destroy(mdc_head_trainer* t) {
    if (!t) return;
    {
        DeviceScope dev(t->device);
        t->release();
        for (void* p : {(void*)t->d_z1part, (void*)t->d_dw1part, (void*)t->d_small, (void*)t->d_h, (void*)t->d_dz1, (void*)t->d_dz2, (void*)t->d_loss, (void*)t->d_hit})
            if (p) (void)hipFree(p);
    }
    delete t;
}

}  // extern "C"
