// What the two training files share (train.hip: the nets the reference trains; head_train.hip: the dense head of VT-CNN2):
// the Dropout mask generator that include/mdc.h states under mdc_trainer_set_dropout, the checked batch index, the wave sum
// whose result is the same bits in every lane, and TensorFlow's Adam update.  `St` is the file's device state record: it has
// `iterations` (Adam's step count) and `bad_indices`.  This is the device half; the host half of what they share -- the parameter
// bank and the bodies of the set / get / read entries -- is train_host.h / train_host.hip.
#pragma once
#include "dense_chain_common.h"      // mdc_internal.h, f32x4, row_allreduce (the 16-lane DPP butterflies)
#include "mdc_fmix32.h"

namespace mdc {

namespace {

constexpr float kKerasEps = 1e-7f;   // K.epsilon()

// The optional Dropout's counter-based generator (include/mdc.h, mdc_trainer_set_dropout; oracle/oracle_train.py restates it):
// keep an element iff fmix32(k_frame + element * 0xC2B2AE35) >= thr, k_frame = fmix32(k_step ^ (frame * 0x85EBCA6B + site)),
// k_step = fmix32(seed + 0x9E3779B9 * (step + 1)); step = Adam's iteration count, read from the device (a replayed hipGraph
// draws new masks at every step), frame = the frame's index in the data set (a frame's mask does not depend on its batch).
struct DropArgs { unsigned seed, thr; float inv; };      // (fmix32: mdc_fmix32.h)
template <class St>
__device__ __forceinline__ unsigned drop_step_key(const DropArgs& d, const St* st) {
    return fmix32(d.seed + 0x9E3779B9u * (unsigned)(st->iterations + 1));
}
__device__ __forceinline__ unsigned drop_frame_key(unsigned kstep, long frame, unsigned site) {
    return fmix32(kstep ^ ((unsigned)frame * 0x85EBCA6Bu + site));
}
__device__ __forceinline__ bool drop_keep(unsigned kframe, unsigned element, unsigned thr) {
    return fmix32(kframe + element * 0xC2B2AE35u) >= thr;
}

// The frame a batch position names, or -1 if that is no frame of the caller's buffers (a shuffle index out of range): such a
// position is SKIPPED -- all-zero samples and targets contribute nothing to loss or gradient below -- and counted, once, by the
// lane `count_it` names; mdc_trainer_read turns the count into an error.  An unchecked index would be a GPU fault instead.
template <class St>
__device__ __forceinline__ long frame_index(const int* __restrict__ order, long first, int i, long n_frames, St* st, bool count_it) {
    const long idx = order ? (long)order[first + i] : first + i;
    if ((unsigned long)idx < (unsigned long)n_frames) return idx;
    if (count_it) atomicAdd(&st->bad_indices, 1u);
    return -1;
}

// Sum over the wave, the same bits in every lane: the DPP butterfly over each 16-lane row (no LDS crossbar: __shfl_xor compiles to
// ds_bpermute_b32, six dependent LDS round trips per sum), then the four row sums through scalar registers in a fixed order.
__device__ __forceinline__ float wave_allsum(float v) {
    v = row_allreduce(v, [](float a, float b) { return a + b; });
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16)),
                r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return (r0 + r1) + (r2 + r3);
}

// TensorFlow 2.4's Adam (optimizer_v2/adam.py -> ApplyAdam), all f32: update number t = iterations + 1,
//     alpha = lr sqrt(1 - beta2^t) / (1 - beta1^t);  m += (g - m)(1 - beta1);  v += (g g - v)(1 - beta2);  w -= m alpha / (sqrt(v) + eps)
// (eps is not scaled by the bias correction).  The one statement of it for both training files.
__device__ __forceinline__ float adam_alpha(float lr, float beta1, float beta2, long long update) {
    const float t = (float)update;
    return lr * sqrtf(1.f - powf(beta2, t)) / (1.f - powf(beta1, t));
}
__device__ __forceinline__ void adam_update(float g, float& m, float& v, float& w, float alpha, float beta1, float beta2, float eps) {
    m = m + (g - m) * (1.f - beta1);
    v = v + (g * g - v) * (1.f - beta2);
    w -= (m * alpha) / (sqrtf(v) + eps);
}

}  // namespace

}  // namespace mdc
