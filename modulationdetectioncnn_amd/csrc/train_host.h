// The host half of what the two training files share (train_common.h holds the device half): the parameter bank that mdc_trainer
// and mdc_head_trainer both are, and the bodies of the entry points that only touch it (train_host.hip).  Every body takes the
// name of the entry the caller called as `who`, so that its error texts keep naming that function; none of this is extern "C".
#pragma once
#include "mdc_internal.h"

namespace mdc {

// Flat f32 parameter vector in Keras' layouts, layer by layer (kernel, bias), three times over for Adam's moments and the last
// gradient, plus the file's device state record (TrainState / HeadState: `long long iterations` first, statistics behind it).
struct ParamBank {
    int device = 0;
    int nlayers = 0;
    size_t nk[4]{}, nb[4]{};
    size_t off_k[4]{}, off_b[4]{};      // offsets into the flat parameter vector
    size_t P = 0;
    bool have[4]{};                     // layer's weights were set
    float lr = 1e-3f, beta1 = 0.9f, beta2 = 0.999f, eps = 1e-7f;      // keras.optimizers.Adam() defaults = the .h5 files' training_config
    float* d_params = nullptr;   // [P] master weights
    float* d_m = nullptr;        // [P] Adam first moment
    float* d_v = nullptr;        // [P] Adam second moment
    float* d_grad = nullptr;     // [P] gradient of the last batch's mean loss
    void* d_state = nullptr;     // the state record

    void layout();                                        // off_k / off_b / P from nlayers, nk, nb
    int alloc(const char* who, size_t state_bytes);       // the four vectors and the record, zeroed, on the current device
    void release();                                        // ... and back (the current device is the bank's)
};

// False, with `who: cannot select device N` as the error, if the scope could not make its device current.
bool device_selected(const char* who, const DeviceScope& dev);

int bank_set_adam(const char* who, ParamBank* b, float lr, float beta1, float beta2, float eps);
int bank_set_tensor(const char* who, ParamBank* b, int which, int layer, const float* kernel_host, size_t kernel_elems, const float* bias_host,
                    size_t bias_elems, hipStream_t s);
int bank_get_tensor(const char* who, ParamBank* b, int which, int layer, float* kernel_host, size_t kernel_elems, float* bias_host, size_t bias_elems,
                    hipStream_t s);
int bank_set_iterations(const char* who, ParamBank* b, int64_t iterations, hipStream_t s);
// Copies the state record (state_bytes) to state_host and, if reset, zeroes it from stats_offset on: the statistics, not
// `iterations`, which is optimizer state.
int bank_read_state(const char* who, ParamBank* b, int reset, void* state_host, size_t state_bytes, size_t stats_offset, hipStream_t s);
// The arguments of one training or evaluation call: weights set, the range [first, first + count) sane and, without a shuffle,
// inside the buffers.  samples / units: the caller's words for x and for what it counts ("frames" / "frames", "features" / "rows").
int bank_check_batch(const char* who, const ParamBank* b, const char* samples, const char* units, const float* x, const float* y, int64_t n,
                     const int32_t* order, int64_t first, int64_t count);

}  // namespace mdc
