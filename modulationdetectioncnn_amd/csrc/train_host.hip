// Host bookkeeping of a training session, once for train.hip and head_train.hip (train_host.h): no kernel lives here.
#include "train_host.h"

#include <cstddef>

namespace mdc {

void ParamBank::layout() {
    size_t off = 0;
    for (int l = 0; l < nlayers; ++l) {
        off_k[l] = off; off += nk[l];
        off_b[l] = off; off += nb[l];
    }
    P = off;
}

int ParamBank::alloc(const char* who, size_t state_bytes) {
    const size_t pb = P * sizeof(float);
    if (hipMalloc(&d_params, pb) != hipSuccess || hipMalloc(&d_m, pb) != hipSuccess || hipMalloc(&d_v, pb) != hipSuccess ||
        hipMalloc(&d_grad, pb) != hipSuccess || hipMalloc(&d_state, state_bytes) != hipSuccess) {
        set_error("%s: out of device memory", who);
        return MDC_ENOMEM;
    }
    if (hipMemset(d_params, 0, pb) != hipSuccess || hipMemset(d_m, 0, pb) != hipSuccess || hipMemset(d_v, 0, pb) != hipSuccess ||
        hipMemset(d_grad, 0, pb) != hipSuccess || hipMemset(d_state, 0, state_bytes) != hipSuccess) {
        set_error("%s: hipMemset failed", who);
        return MDC_EIO;
    }
    return MDC_OK;
}

void ParamBank::release() {
    for (void* p : {(void*)d_params, (void*)d_m, (void*)d_v, (void*)d_grad, d_state})
        if (p) (void)hipFree(p);
    d_params = d_m = d_v = d_grad = nullptr;
    d_state = nullptr;
}

bool device_selected(const char* who, const DeviceScope& dev) {
    if (!dev.ok) set_error("%s: cannot select device %d", who, dev.want);
    return dev.ok;
}

int bank_set_adam(const char* who, ParamBank* b, float lr, float beta1, float beta2, float eps) {
    if (!b) { set_error("null trainer"); return MDC_EINVAL; }
    if (!(lr > 0.f) || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps >= 0.f)) {
        set_error("%s: need lr > 0, 0 <= beta < 1, eps >= 0", who);
        return MDC_EINVAL;
    }
    b->lr = lr; b->beta1 = beta1; b->beta2 = beta2; b->eps = eps;
    return MDC_OK;
}

namespace {

// which: 0 weights, 1 Adam m, 2 Adam v, 3 gradient of the last batch
float* bank_vec(ParamBank* b, int which) {
    switch (which) {
        case MDC_TRAIN_WEIGHTS: return b->d_params;
        case MDC_TRAIN_ADAM_M:  return b->d_m;
        case MDC_TRAIN_ADAM_V:  return b->d_v;
        case MDC_TRAIN_GRADIENT: return b->d_grad;
        default: return nullptr;
    }
}

// One (kernel, bias) pair between the host and vector `which`, either way; the checks in the order null, layer, `which`, sizes.
int bank_tensor(const char* who, ParamBank* b, int which, int layer, float* kernel_host, size_t kernel_elems, float* bias_host, size_t bias_elems,
                bool set, hipStream_t s) {
    if (!b || !kernel_host || !bias_host) { set_error("%s: null argument", who); return MDC_EINVAL; }
    if (layer < 0 || layer >= b->nlayers) { set_error("%s: layer %d out of range 0..%d", who, layer, b->nlayers - 1); return MDC_EINVAL; }
    float* vec = bank_vec(b, which);
    if (set && (!vec || which == MDC_TRAIN_GRADIENT)) { set_error("%s: `which` must be MDC_TRAIN_WEIGHTS, _ADAM_M or _ADAM_V", who); return MDC_EINVAL; }
    if (!vec) { set_error("%s: unknown tensor kind %d", who, which); return MDC_EINVAL; }
    if (kernel_elems != b->nk[layer] || bias_elems != b->nb[layer]) {
        set_error("%s: layer %d holds kernel %zu / bias %zu elements, got %zu / %zu", who, layer, b->nk[layer], b->nb[layer], kernel_elems, bias_elems);
        return MDC_EINVAL;
    }
    DeviceScope dev(b->device);
    if (!device_selected(who, dev)) return MDC_EIO;
    const hipMemcpyKind kind = set ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    float *dk = vec + b->off_k[layer], *db = vec + b->off_b[layer];
    MDC_HIP(hipMemcpyAsync(set ? dk : kernel_host, set ? kernel_host : dk, kernel_elems * sizeof(float), kind, s));
    MDC_HIP(hipMemcpyAsync(set ? db : bias_host, set ? bias_host : db, bias_elems * sizeof(float), kind, s));
    MDC_HIP(hipStreamSynchronize(s));      // the host buffers are the caller's again on return
    if (set && which == MDC_TRAIN_WEIGHTS) b->have[layer] = true;
    return MDC_OK;
}

}  // namespace

int bank_set_tensor(const char* who, ParamBank* b, int which, int layer, const float* kernel_host, size_t kernel_elems, const float* bias_host,
                    size_t bias_elems, hipStream_t s) {
    return bank_tensor(who, b, which, layer, const_cast<float*>(kernel_host), kernel_elems, const_cast<float*>(bias_host), bias_elems, true, s);
}

int bank_get_tensor(const char* who, ParamBank* b, int which, int layer, float* kernel_host, size_t kernel_elems, float* bias_host, size_t bias_elems,
                    hipStream_t s) {
    return bank_tensor(who, b, which, layer, kernel_host, kernel_elems, bias_host, bias_elems, false, s);
}

int bank_set_iterations(const char* who, ParamBank* b, int64_t iterations, hipStream_t s) {
    if (!b || iterations < 0) { set_error("%s: bad argument", who); return MDC_EINVAL; }
    DeviceScope dev(b->device);
    if (!device_selected(who, dev)) return MDC_EIO;
    const long long v = iterations;      // the first field of either state record
    MDC_HIP(hipMemcpyAsync(b->d_state, &v, sizeof(v), hipMemcpyHostToDevice, s));
    MDC_HIP(hipStreamSynchronize(s));
    return MDC_OK;
}

int bank_read_state(const char* who, ParamBank* b, int reset, void* state_host, size_t state_bytes, size_t stats_offset, hipStream_t s) {
    if (!b) { set_error("null trainer"); return MDC_EINVAL; }
    DeviceScope dev(b->device);
    if (!device_selected(who, dev)) return MDC_EIO;
    MDC_HIP(hipMemcpyAsync(state_host, b->d_state, state_bytes, hipMemcpyDeviceToHost, s));
    MDC_HIP(hipStreamSynchronize(s));
    if (reset) {
        MDC_HIP(hipMemsetAsync(static_cast<char*>(b->d_state) + stats_offset, 0, state_bytes - stats_offset, s));
        MDC_HIP(hipStreamSynchronize(s));
    }
    return MDC_OK;
}

int bank_check_batch(const char* who, const ParamBank* b, const char* samples, const char* units, const float* x, const float* y, int64_t n,
                     const int32_t* order, int64_t first, int64_t count) {
    if (!b) { set_error("%s: null trainer", who); return MDC_EINVAL; }
    for (int l = 0; l < b->nlayers; ++l)
        if (!b->have[l]) { set_error("%s: layer %d has no weights (set MDC_TRAIN_WEIGHTS of every layer first)", who, l); return MDC_ESTATE; }
    if (first < 0 || count < 0) { set_error("%s: negative range", who); return MDC_EINVAL; }
    if (count > (int64_t)1 << 30) { set_error("%s: at most 2^30 %s per call", who, units); return MDC_EINVAL; }
    if (count > 0 && (!x || !y)) { set_error("%s: null %s or targets", who, samples); return MDC_EINVAL; }
    if ((reinterpret_cast<uintptr_t>(x) & 15) != 0) { set_error("%s: %s must be 16-byte aligned", who, samples); return MDC_EINVAL; }
    if (n < 0) { set_error("%s: negative n_%s", who, units); return MDC_EINVAL; }
    // without a shuffle the positions ARE the frames / rows: checked here; with one, its VALUES are checked on the device (frame_index)
    if (!order && (first > n || count > n - first)) {      // (first + count may not be representable)
        set_error("%s: %lld %s from %lld on lie outside the %lld of the buffers", who, (long long)count, units, (long long)first, (long long)n);
        return MDC_EINVAL;
    }
    return MDC_OK;
}

}  // namespace mdc
