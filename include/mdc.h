/* mdc.h -- C ABI of libmdc.so: MI355X (gfx950) inference path for the VT-CNN2-family
 * modulation classifiers of peteroh23/ModulationDetectionCNN.
 *
 * The reference has no FFI/plugin interface; its boundary is the Keras object surface
 * (citations into /root/reference):
 *     model = models.Sequential(); model.add(...)      cnn.py:104-115, CNN.ipynb cell 6,
 *                                                      RML2016.10a_VTCNN2_example.ipynb:229-243
 *     model.load_weights(filepath)                     cnn.py:147, CNN.ipynb cell 8
 *     model.predict(X, batch_size=...)                 cnn.py:198, cnn.py:237, CNN.ipynb cell 12
 *     Model(inputs, outputs=model.layers[i].output)    CNN.ipynb cell 17 (layer taps)
 *     int(np.argmax(test_Y_hat[i,:]))                  cnn.py:209 (first maximum wins)
 * Each entry point below names the call it replaces.  INTEGRATION.md shows the ctypes
 * binding (modulationdetectioncnn_amd/_cabi.py is that binding).
 *
 * Conventions: plain C types only; every function returns 0 on success or a negative
 * errno-style code and sets a thread-local message (mdc_last_error); nothing aborts,
 * nothing throws across the boundary.  All device buffers belong to the caller; the
 * library owns only the packed weights.  mdc_forward is asynchronous on the caller's HIP
 * stream and performs no device synchronisation.  A finalized model is immutable and
 * mdc_forward on it is re-entrant (one model per device; any number of streams and host threads; with
 * mdc_set_profiling on, the per-launch event lists are kept under a mutex, so that stays true).  Every entry point
 * that touches a device selects the model's device for the duration of the call and restores the caller's.
 * The library is built with C++ exceptions enabled internally: an allocation failure inside it (weight copies,
 * packing buffers, event lists) is caught at the boundary and returned as MDC_ENOMEM.
 */
#ifndef MDC_H
#define MDC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* libmdc.so is built with -fvisibility=hidden: the entry points below are its ONLY dynamic symbols
 * (tests/test_cabi.py compares `nm -D --defined-only` with this header, both ways). */
#if defined(__GNUC__) || defined(__clang__)
#define MDC_API __attribute__((visibility("default")))
#else
#define MDC_API
#endif

#define MDC_ABI_VERSION 5   /* 2: mdc_forward_iq_u8 takes hop + workspace; mdc_confusion_binned, mdc_iq_u8_windows
                               3: mdc_topology.reserved[0] is a validated option word (no bit defined: must be 0);
                                  mdc_iq_u8_windows wants 2-byte aligned input; the library reads no environment
                               4: MDC_KIND_VTCNN2 at MDC_FP8 keeps E4M3 features (its workspace per frame shrinks from
                                  22,144 to 11,584 bytes: ask mdc_workspace_bytes); MDC_OPT_FP8_BF16_FEATURES restores
                                  ABI 3's numerics and workspace
                               5: the training step (mdc_trainer_*, mdc_train_batch): additive; later, also additive:
                                  mdc_forward_checked / mdc_predict_host_checked, MDC_NONFINITE_* (non-finite frames);
                                  mdc_iq_u8_windows_norm / mdc_predict_host_iq_u8_norm (level-normalised raw I/Q);
                                  mdc_iq_windows / mdc_iq_windows_norm / mdc_predict_host_iq / mdc_predict_host_iq_norm
                                  (signed 8- and 16-bit sample formats, MDC_IQ_*, mdc_iq_window_stats64);
                                  mdc_iq_ddc / mdc_iq_ddc_out_count / mdc_iq_ddc_nco_table (frequency shift, low-pass and
                                  decimation of a raw capture, exact integers);
                                  mdc_iq_resample / mdc_iq_resample_out_count (the same with a rational factor L/D);
                                  mdc_iq_spectrogram / mdc_iq_spectrogram_rows (averaged power spectra of a raw capture);
                                  mdc_iq_line_spectrum (the same of the capture's envelope, square or fourth power: the
                                  spectral lines at the symbol rate and at 2 / 4 times the carrier offset);
                                  mdc_iq_spectrum_quantiles (order statistics of a spectrogram along time, per bin);
                                  mdc_iq_spectrogram_components / mdc_iq_spectrogram_components_workspace, mdc_iq_component
                                  (connected components of a thresholded spectrogram: boxes in time and frequency);
                                  mdc_iq_spectrogram_cfar (a local order-statistic noise floor per cell, and the ratio to it);
                                  mdc_iq_extract / mdc_iq_extract_plan / mdc_iq_extract_plan_bytes, mdc_iq_extract_job,
                                  mdc_iq_extract_filter (K stretches of a capture through mdc_iq_resample's chain in one launch);
                                  mdc_iq_line_spectra / mdc_iq_line_spectra_rows, mdc_iq_line_job (the line spectra of K stretches
                                  at several orders, and their float64 means, in one call); mdc_iq_find_lines, mdc_iq_line_band,
                                  mdc_iq_line_record (the line search of S spectra on the device);
                                  mdc_iq_balance / mdc_iq_balance_stats / mdc_iq_balance_blocks, mdc_iq_balance_coeffs (a
                                  receiver's I/Q imbalance and DC offset, measured and corrected in exact integers);
                                  mdc_iq_cf32_histogram / mdc_iq_cf32_quantize (a complex float32 capture: the exponent
                                  histogram of its components, and one exact rounding into an MDC_IQ_CI16 stream);
                                  mdc_iq_synth_plan / mdc_iq_synth_plan_bytes / mdc_iq_synth_frames, mdc_iq_synth_class (labelled
                                  I/Q frames of a balanced modulation x SNR grid, synthesised on the device in exact integers);
                                  mdc_iq_synth_frames_faded, mdc_iq_synth_fading, mdc_iq_synth_path (the same frames through a
                                  frequency-selective Rician channel);
                                  mdc_iq_synth_scene / mdc_iq_synth_scene_bytes / mdc_iq_synth_scene_hops / mdc_iq_synth_capture /
                                  mdc_iq_synth_capture_workspace_bytes, mdc_iq_synth_emitter (a scene of bursty and hopping
                                  emitters rendered into one wideband capture, with the draws its truth table needs);
                                  mdc_head_trainer_* / mdc_head_train_batch (head training: the dense layers of VT-CNN2 on
                                  precomputed feature rows) */

/* error codes (negative errno values) */
#define MDC_OK        0
#define MDC_EINVAL   (-22)
#define MDC_ENOMEM   (-12)
#define MDC_ENODEV   (-19)
#define MDC_ENOTSUP  (-95)
#define MDC_EIO      (-5)     /* a HIP runtime call failed; see mdc_last_error() */
#define MDC_ESTATE   (-1)     /* call out of order (e.g. forward before finalize) */

/* Topology families.  Input is always (n, 2, 128) float32 I/Q. */
enum {
    MDC_KIND_DEPLOYED = 1,  /* CNN.ipynb cell 6: pad(0,1) Conv2D(F,(1,2)) relu Flatten Dense(C,relu) softmax;
                               F = filters in {3,10}, C = 3.  Layers: 0 conv, 1 dense.             */
    MDC_KIND_VTCNN2   = 2,  /* RML2016.10a_VTCNN2_example.ipynb:229-243: pad(0,2) Conv(256,1x3) relu
                               pad(0,2) Conv(80,2x3) relu Flatten Dense(256,relu) Dense(C) softmax.
                               Layers: 0 conv1, 1 conv2, 2 dense1, 3 dense2.  C <= 16.             */
    MDC_KIND_CNNPY    = 3   /* cnn.py:104-115 literal model (H=1,W=2,C=128 under channels_last):
                               pad(0,1) Conv2D(F,(1,2)) relu Flatten Dense(D,relu) Dense(C) softmax.
                               Layers: 0 conv, 1 dense1, 2 dense2.                                 */
};

/* Arithmetic type of the matrix products (accumulation is always f32).  MDC_BF16: MDC_KIND_VTCNN2 (both convs'
 * and dense1's operands) and MDC_KIND_DEPLOYED (the dense layer's operands; the conv stays f32; no layer taps).
 * MDC_KIND_VTCNN2 in the 16-bit modes keeps its activations and features multiplied by 2^-32 internally (an exact
 * power of two; the ReLU then rides in the bf16 conversion's clamp bit): conv1 / conv2 activations of 2^32 (4.3e9)
 * and beyond saturate, those below 2^-94 flush to zero -- I/Q samples of order 1e-2 sit in the middle of that range.
 * MDC_KIND_DEPLOYED does the same with its conv taps and bias at MDC_F32 and MDC_BF16 (the ReLU rides in the second
 * fma's / the conversion's clamp bit; dense weights carry the 2^+32): bit-identity to Keras' operation order holds for
 * conv activations in [2^-94, 2^32) -- at 2^32 and beyond they saturate at 2^32 instead of growing on, below 2^-94 the
 * scaled value is an f32 denormal (bits lost, then zero).  A frame holding a NaN or +-Inf sample gets no NaN row from
 * mdc_forward (tests/test_deployed_gpu.py pins that it stays within its frame): mdc_forward_checked flags such frames and,
 * asked to, gives them Keras' NaN row.  The MDC_TAP_CONV / MDC_TAP_FLAT taps of the deployed nets come
 * from a kernel that reads the UNSCALED table and rectifies with fmaxf: outside that range a tap and the probabilities of
 * the same frame can disagree.
 * MDC_F16: MDC_KIND_DEPLOYED only -- as MDC_BF16 there, with IEEE f16 operands and the conv itself in packed f16
 * (11 significant bits instead of 8, but conv outputs must stay below 65,504).
 * MDC_FP8: MDC_KIND_VTCNN2 -- conv2 on the block-scaled e4m3 MFMA, its features handed to dense1 as E4M3 bytes (conv1
 * and dense1's arithmetic as in MDC_BF16; see MDC_OPT_FP8_BF16_FEATURES) -- and
 * MDC_KIND_DEPLOYED -- as MDC_BF16 there with e4m3 operands (BASELINE configs[4] read literally); the activations are
 * scaled for the largest |sample| given with mdc_set_fp8_input_absmax -- beyond it they saturate. */
enum { MDC_F32 = 0, MDC_BF16 = 1, MDC_FP8 = 2, MDC_F16 = 3 };

/* Layer taps of CNN.ipynb cell 17.  tap_dev receives, per frame:
 *   MDC_TAP_CONV   model4: last conv+ReLU output in the reference's layout
 *                  (deployed: (2,129,F) channels_last; vtcnn2: (80,132) channels_first)
 *   MDC_TAP_FLAT   model3: Flatten output (same values, same order as CONV)
 *   MDC_TAP_DENSE  model2: output of the last Dense before softmax
 *                  (deployed: post-ReLU (C); vtcnn2/cnnpy: logits (C))
 *   MDC_TAP_HIDDEN vtcnn2/cnnpy only: Dense1+ReLU output                                   */
enum { MDC_TAP_NONE = 0, MDC_TAP_CONV = 1, MDC_TAP_FLAT = 2, MDC_TAP_DENSE = 3, MDC_TAP_HIDDEN = 4 };

typedef struct mdc_topology {
    int32_t kind;        /* MDC_KIND_*                                                       */
    int32_t filters;     /* deployed: F (3 or 10); cnnpy: F (10); vtcnn2: ignored (256/80)    */
    int32_t hidden;      /* cnnpy: D (10); vtcnn2: ignored (256); deployed: ignored           */
    int32_t classes;     /* C                                                                */
    int32_t reserved[4]; /* [0]: option bits MDC_OPT_* (0 = defaults); [1..3] must be 0      */
} mdc_topology;

/* Option bits (mdc_topology.reserved[0]; validated by mdc_create, fixed for the model's life).  Every kernel evaluates
 * the layers in Keras' operation order whatever the bits say (round 2's re-associated conv of the 10-filter net and the
 * bit that switched it off are gone: the ReLU now rides in the fma's clamp bit, which is faster AND exact).
 * MDC_OPT_FP8_BF16_FEATURES (MDC_KIND_VTCNN2, honoured at MDC_FP8 only, refused at any other dtype): keep the conv2
 * features between the conv kernel and dense1 in bf16, as the library did up to ABI 3.  Default since ABI 4: E4M3 bytes
 * with one power-of-two scale per tensor (half the feature traffic of both kernels; dense1 converts them back to bf16
 * exactly and keeps bf16 weights, so only the features' own rounding -- 3 significant bits + hidden one instead of
 * 7 + 1 -- changes: tests/test_label_agreement_gpu.py holds the same label floors for both). */
#define MDC_OPT_FP8_BF16_FEATURES 1
#define MDC_OPT_ALL 1

typedef struct mdc_model mdc_model;   /* opaque, owned by the library */

MDC_API int mdc_abi_version(void);

/* models.Sequential() + model.add(...): describe the net.  `device` is the HIP ordinal. */
MDC_API int mdc_create(const mdc_topology* topo, int device, mdc_model** out);

/* Number of weighted layers and the element counts load_weights must supply for each. */
MDC_API int mdc_num_layers(const mdc_model* m);
MDC_API int mdc_layer_sizes(const mdc_model* m, int layer, size_t* kernel_elems, size_t* bias_elems);

/* model.load_weights(): one call per weighted layer, host pointers in the Keras layout
 * (deployed/cnnpy conv: HWIO; vtcnn2 conv: OIHW; dense: (in, out) with `in` in the
 * reference's Flatten order).  The data is copied; the caller keeps ownership.            */
MDC_API int mdc_set_weights(mdc_model* m, int layer, const float* kernel_host, size_t kernel_elems,
                    const float* bias_host, size_t bias_elems);

/* Pack the weights into the kernels' register/LDS/MFMA layouts and upload them.
 * After this the model is immutable.  dtype: MDC_F32 | MDC_BF16 | MDC_FP8. */
MDC_API int mdc_finalize(mdc_model* m, int dtype);

/* MDC_FP8 only, before mdc_finalize: the largest |I/Q sample| the caller will feed (default 0.02, the scale of the
 * reference's bundled frames).  It fixes the power-of-two scale of the fp8 activations. */
MDC_API int mdc_set_fp8_input_absmax(mdc_model* m, float absmax);

/* MDC_KIND_VTCNN2 at MDC_FP8 with E4M3 features (the default), before mdc_finalize: the largest conv2 + ReLU output the
 * features must represent, e.g. twice the largest MDC_TAP_CONV value a bf16 / f32 forward of a sample batch produced
 * (calibration).  It fixes the power-of-two scale of the E4M3 bytes: values up to 2 x absmax keep their e4m3 precision,
 * larger ones saturate.  Not called: the library estimates it from the weights (12 sigma of the conv2 sum for independent
 * samples of rms fp8_input_absmax / 4).  Added in ABI 5. */
MDC_API int mdc_set_fp8_feature_absmax(mdc_model* m, float absmax);

/* Bytes of caller-owned device scratch ONE mdc_forward call of n frames needs (0 for deployed / cnnpy).
 * MDC_KIND_VTCNN2 keeps a call's conv2 features there: n rounded up to 256 frames x (10,560 features x 2 B in the
 * bf16 / fp8 modes, 4 B at f32, + 1 KiB of hidden layer) = 22,144 B (f32: 43,264 B) per frame -- 1.45 GB for a
 * 65,536-frame call, 23.2 GB for a 2^20-frame one.  The cost is PER CONCURRENT CALL: forwards enqueued on different
 * streams must not share a workspace.  A caller bounds it by splitting a batch into several calls (results do not
 * depend on the split; 65,536 frames per call already fill the chip 16 times over and cost 1.5 % against one
 * 2^20-frame call); modulationdetectioncnn_amd.VTCNN2 does that by default. */
MDC_API size_t mdc_workspace_bytes(const mdc_model* m, int64_t n);

/* model.predict(X) (+ np.argmax): x_dev (n,2,128) f32 contiguous on the model's device.
 * probs_dev (n,C) f32 or NULL; labels_dev (n) int32 or NULL (first-max tie-break);
 * tap_dev NULL unless tap != MDC_TAP_NONE.  Enqueued on hip_stream (NULL = null stream). */
MDC_API int mdc_forward(const mdc_model* m, const void* x_dev, int64_t n,
                float* probs_dev, int32_t* labels_dev,
                float* tap_dev, int tap,
                void* workspace_dev, size_t workspace_bytes,
                void* hip_stream);

/* ---- non-finite input frames (cnn.py:153, 198) -----------------------------------------------------------------------
 * What Keras does with a frame holding a NaN or +-Inf sample: a NaN sample always gives an all-NaN softmax row (NaN x w is
 * NaN, np.maximum and TF's ReLU pass it on, and Dense mixes every position into every unit); np.argmax of that row is 0 and
 * model.evaluate's mean loss is nan.  A +-Inf sample almost always gives one too (Inf x 0 taps, Inf - Inf in the Dense sums,
 * the softmax's x - max), but a -Inf conv output that the ReLU turns into 0 can leave Keras' row finite.  mdc_forward
 * returns finite rows for all such frames (the 2^-32 scaling and the ReLU in the clamp bit above).
 *
 * mdc_forward_checked is mdc_forward for f32 frames plus a check of every sample of every frame:
 *   nonfinite_dev (n) uint8, REQUIRED: 1 if frame i holds a NaN or +-Inf sample, else 0 (finite extremes -- +-FLT_MAX,
 *                 denormals, -0.0 -- are finite);
 *   nonfinite_count_dev int64, may be NULL: += the number of such frames (caller-zeroed; accumulates across calls);
 *   policy MDC_NONFINITE_REPORT: probs and labels are bit-identical to mdc_forward for EVERY frame, bad ones included;
 *          MDC_NONFINITE_PROPAGATE: each flagged frame gets an all-NaN probability row and label 0 (np.argmax of that row);
 *          every other frame is bit-identical to mdc_forward.  PROPAGATE treats every non-finite sample alike, so on the
 *          rare +-Inf frame whose Keras row stays finite (see above) it gives NaN where Keras does not.
 * Every kind and every dtype mdc_finalize accepts, MDC_OPT_FP8_BF16_FEATURES included; no layer taps.  Validation as
 * mdc_forward; an unknown policy or a NULL nonfinite_dev (n > 0) is MDC_EINVAL.  mdc_workspace_bytes is unchanged (the
 * flags live in the caller's buffer).  The call only enqueues on hip_stream and can be captured in a hipGraph like
 * mdc_forward.  MDC_KIND_DEPLOYED: the forward kernels check the samples they already hold and write flags, count and NaN
 * rows themselves (one launch, as mdc_forward); MDC_KIND_VTCNN2 / MDC_KIND_CNNPY: the forward, then one more launch that
 * reads the frames, writes the flags and, under PROPAGATE, the NaN rows.  In libmdc_alt.so the checked entries always run
 * the product kernels (no alternate is selected for them).  Raw uint8 input cannot be non-finite: mdc_forward_iq_u8
 * and mdc_predict_host_iq_u8 have no checked twin. */
enum { MDC_NONFINITE_REPORT = 0, MDC_NONFINITE_PROPAGATE = 1 };

MDC_API int mdc_forward_checked(const mdc_model* m, const void* x_dev, int64_t n,
                float* probs_dev, int32_t* labels_dev,
                void* workspace_dev, size_t workspace_bytes,
                uint8_t* nonfinite_dev, int64_t* nonfinite_count_dev,
                int policy, void* hip_stream);

/* mdc_predict_host with the same check: nonfinite_host (n) uint8 is REQUIRED; *nonfinite_count (host, may be NULL) is SET
 * to the number of flagged frames, not accumulated.  Results are bit-identical to mdc_forward_checked on the same frames,
 * whatever the chunk. */
MDC_API int mdc_predict_host_checked(mdc_model* m, const float* x_host, int64_t n,
                float* probs_host, int32_t* labels_host, uint8_t* nonfinite_host,
                int64_t* nonfinite_count, int policy, int64_t chunk_frames);

/* ---- callers either side of the forward -------------------------------------------

 * Q6.12 integer forward of a DEPLOYED model: the arithmetic of the reference's FPGA datapath
 * (cnn_test_latest1.sv:642-675 bit selections, 18-bit wrap, 32-bit dense accumulators, sv:293-343, 171-176), for
 * validating ROM tables / test vectors written by the float2fix exporter (CNN.ipynb cells 23-24).  The integer
 * tables are made from the model's weights at mdc_finalize (float2fix: trunc(v * 4096)).
 * x_dev: (n,2,128) f32 frames (quantised on load, x_is_q612 = 0) or int32 Q6.12 words (x_is_q612 = 1).
 * dense_dev (n,C) int32 = post-ReLU class sums, value/4096 (or NULL); labels_dev (n) int32 first maximum (or NULL).
 * Input domain: an integer word is taken modulo 2^18 (bits 18..31 are ignored, whatever they hold).  A float sample v
 * with |v| < 2^19 becomes trunc(v * 4096) wrapped to 18 bits, exactly as float2fix writes it.  A frame that holds a
 * sample with |v| >= 2^19, a NaN or an infinity gets unspecified class sums and a label in [0, C); such a frame never
 * affects another frame's results.  The kernel exists for F = 3 and F = 10 filters, the only deployed topologies
 * mdc_create admits (any other F is MDC_ENOTSUP there, so no such model reaches this call). */
MDC_API int mdc_forward_q612(const mdc_model* m, const void* x_dev, int x_is_q612, int64_t n,
                     int32_t* dense_dev, int32_t* labels_dev, void* hip_stream);

/* Confusion counts of cnn.py:205-216 / 242-255 on the device: counts_dev[t*classes + p] += 1 for every i with
 * truth_dev[i] == t and pred_dev[i] == p (int64, caller-zeroed, accumulates across calls).  Pairs with a label
 * outside [0,classes) are added to *bad_dev instead (may be NULL).  classes <= 32.  Runs on the current device. */
MDC_API int mdc_confusion(const int32_t* truth_dev, const int32_t* pred_dev, int64_t n, int classes,
                  int64_t* counts_dev, int64_t* bad_dev, void* hip_stream);

/* The per-SNR evaluation loop of cnn.py:228-259 in ONE launch: bin_dev[i] in [0,bins) says which SNR (or any other
 * grouping) frame i belongs to, and counts_dev[(b*classes + t)*classes + p] += 1 -- a (bins, classes, classes) int64
 * histogram, caller-zeroed; acc[b] = trace / sum of slice b (cnn.py:257-259).  Entries with a label or bin out of
 * range go to *bad_dev (may be NULL).  classes <= 32, bins <= 65536.  Runs on the current device. */
MDC_API int mdc_confusion_binned(const int32_t* truth_dev, const int32_t* pred_dev, const int32_t* bin_dev, int64_t n,
                         int classes, int bins, int64_t* counts_dev, int64_t* bad_dev, void* hip_stream);

/* score = model.evaluate(X_test, Y_test, ...)  (cnn.py:153; the reference compiles with loss='categorical_crossentropy' and
 * no metric, so the score is the mean loss): *loss_sum_dev += sum over i of -log(clip(p_i[t_i] / sum_c p_i[c], 1e-7, 1 - 1e-7))
 * with p_i = probs_dev[i*classes ..] (the softmax rows mdc_forward returned) and t_i = truth_dev[i] (the index of the
 * one-hot row's 1) -- Keras' categorical_crossentropy on probabilities.  f64, caller-zeroed, accumulates across calls; the
 * mean is loss_sum / n.  Labels outside [0,classes) are counted in *bad_dev (may be NULL) and add nothing.  classes <= 32.
 * Runs on the current device.  Added in ABI 4 (additive). */
MDC_API int mdc_crossentropy(const float* probs_dev, const int32_t* truth_dev, int64_t n, int classes,
                     double* loss_sum_dev, int64_t* bad_dev, void* hip_stream);

/* Raw SDR bytes -> frames: iq_dev holds n frames of 128 interleaved unsigned 8-bit (I,Q) pairs (256 B/frame, the
 * RTL-SDR format of the front-end in the reference's README.md:5); x_dev (n,2,128) f32 receives
 * ((byte - 127.5) * scale) with I in row 0 and Q in row 1.  Runs on the current device. */
MDC_API int mdc_iq_u8_to_frames(const uint8_t* iq_dev, int64_t n, float scale, float* x_dev, void* hip_stream);

/* Sliding windows over one contiguous capture (the live RTL-SDR stream of README.md:5): window i holds the 128 (I,Q)
 * pairs starting at pair i*hop, i.e. bytes [2*hop*i, 2*hop*i + 256) of iq_dev, which must hold 2*hop*(n-1) + 256 bytes.
 * hop = MDC_HOP_FRAME (128) is mdc_iq_u8_to_frames.  x_dev (n,2,128) f32.  Runs on the current device. */
#define MDC_HOP_FRAME 128
MDC_API int mdc_iq_u8_windows(const uint8_t* iq_dev, int64_t n, int64_t hop, float scale, float* x_dev, void* hip_stream);
/* (iq_dev 2-byte aligned -- whole (I,Q) pairs --, as mdc_forward_iq_u8 requires; otherwise MDC_EINVAL) */

/* Conversion and forward in ONE pass, for the deployed nets (any of their dtypes) and the VT-CNN2 family (f32, bf16,
 * fp8): the forward kernel itself reads the raw bytes (the deployed kernels' loads / LDS-DMA, the VT-CNN2 conv
 * kernels' frame staging) and converts in registers with the arithmetic of mdc_iq_u8_to_frames, so probs/labels are
 * bit-identical to mdc_iq_u8_windows followed by mdc_forward -- with 2*hop (<= 256) instead of 1,024 B of HBM input
 * per window and no frame buffer in between.  n windows, `hop` pairs apart as in mdc_iq_u8_windows (MDC_HOP_FRAME:
 * disjoint 256-byte frames); iq_dev 2-byte aligned (windows at odd hops are not better aligned than that anyway: the
 * kernels use gfx950's unaligned global loads), 2*hop*(n-1) + 256 bytes.  probs_dev (n,C) f32 and labels_dev (n)
 * int32 may each be NULL.  workspace: as mdc_forward (mdc_workspace_bytes(m, n); NULL/0 for the deployed nets).
 * MDC_KIND_CNNPY: MDC_ENOTSUP (use the two calls).  This is the SDR -> classifier hand-off of README.md:5. */
MDC_API int mdc_forward_iq_u8(const mdc_model* m, const uint8_t* iq_dev, int64_t n, int64_t hop, float scale,
                      float* probs_dev, int32_t* labels_dev,
                      void* workspace_dev, size_t workspace_bytes, void* hip_stream);

/* ---- level-normalised windows: DC removal, fixed rms, power (additive in ABI 5) ------------------------------------------
 * mdc_iq_u8_windows / mdc_forward_iq_u8 turn every byte into (byte - 127.5) * scale with ONE scale for the whole capture,
 * but the nets were trained on level-normalised frames (RadioML2016.10a normalises each 128-sample vector's energy; the
 * bundled frames sit at a complex rms of about 7.8e-3), and an RTL-SDR capture has whatever level the tuner gain gave it
 * plus a DC offset.  mdc_iq_u8_windows_norm is mdc_iq_u8_windows with a scale PER WINDOW, chosen so that the window's
 * complex rms sqrt(mean(I^2 + Q^2)) equals `level`, after removing each channel's mean if MDC_IQ_REMOVE_DC is set; it
 * also returns the window's statistics as exact integers, for a power estimate / squelch.
 *
 * Windows are addressed exactly as in mdc_iq_u8_windows: window i covers bytes [2*hop*i, 2*hop*i + 256) of iq_dev, hop in
 * 1..2^24, iq_dev 2-byte aligned (odd hops are supported).  With s = 2*byte - 255 (an odd integer in [-255, 255]):
 *     sum_i, sum_q   sum of s over the window's 128 I bytes / 128 Q bytes
 *     sum_sq         sum of s_I^2 + s_Q^2 over the 128 pairs (<= 16,646,400)
 *     energy  E      with MDC_IQ_REMOVE_DC:  E = 128*sum_sq - sum_i^2 - sum_q^2  ( = 128 * sum |a|^2,  a = s - mean )
 *                    without it:             E = 128*sum_sq                      ( a = s )
 *                    0 <= E <= 128*256*255^2 = 2,130,739,200 < 2^31; computed in integers: all four fields are exact.
 *     x              = a * (128*level / sqrt(E)), I in row 0 and Q in row 1 of the (2,128) frame.  a is exact in f32 (s is
 *                    an integer, the mean a multiple of 1/128); the remaining roundings are the conversion of E, the
 *                    square root, one division and one multiplication, each correctly rounded: |x - exact| <= 2^-21 |exact|.
 *                    A constant window (E == 0) gives an all-zero frame, never NaN or Inf.
 * The window's power relative to a full-scale constant-envelope one is E / (128*255)^2 (10*log10 of it: dBFS).
 * x_dev (n,2,128) f32, 8-byte aligned, or NULL (statistics only); stats_dev (n), 16-byte aligned, or NULL; not both NULL.
 * level must be finite and > 0; flags may hold MDC_IQ_REMOVE_DC only; a NULL iq_dev with n > 0: MDC_EINVAL.  The call only
 * enqueues on hip_stream (no synchronisation, no allocation: capturable in a hipGraph) and runs on the current device, like
 * mdc_iq_u8_windows.  Followed by mdc_forward it serves every kind, MDC_KIND_CNNPY included.
 * MDC_FP8: set mdc_set_fp8_input_absmax to level x the crest factor (peak / rms) the caller expects of its signals; the hard
 * bound on a normalised sample is level * sqrt(128) (one pair carrying the whole window's energy). */
typedef struct mdc_iq_window_stats {   /* 16 B */
    int32_t  sum_i, sum_q;
    uint32_t sum_sq;
    uint32_t energy;
} mdc_iq_window_stats;

#define MDC_IQ_REMOVE_DC 1             /* flags of mdc_iq_u8_windows_norm / mdc_predict_host_iq_u8_norm */

MDC_API int mdc_iq_u8_windows_norm(const uint8_t* iq_dev, int64_t n, int64_t hop, float level, int flags,
                           float* x_dev, mdc_iq_window_stats* stats_dev, void* hip_stream);

/* ---- other sample formats: signed 8- and 16-bit captures (additive in ABI 5) ----------------------------------------------
 * mdc_iq_windows / mdc_iq_windows_norm are mdc_iq_u8_windows / mdc_iq_u8_windows_norm for a capture in one of three integer
 * sample formats, interleaved I0 Q0 I1 Q1 ...; one (I,Q) PAIR is 2 / 2 / 4 bytes:
 *     format         integer sample s            plain conversion x (mdc_iq_windows)              full-scale amplitude A
 *     MDC_IQ_CU8     2*byte - 255                (byte - 127.5) * scale  (exactly mdc_iq_u8_windows)   255   RTL-SDR, SigMF cu8
 *     MDC_IQ_CI8     the int8 value              (float)s * scale                                      128   HackRF, SigMF ci8
 *     MDC_IQ_CI16    the int16 value, little-    (float)s * scale                                    32768   USRP sc16, SDRplay,
 *                    endian                                                                                  bladeRF, Airspy, ci16_le
 * Windows are addressed as in mdc_iq_u8_windows: window i is the 128 pairs from pair i*hop on, hop in 1..2^24 (odd hops are
 * supported); iq_dev holds (hop*(n-1) + 128) pairs and is aligned to ONE PAIR (2 / 2 / 4 bytes), otherwise MDC_EINVAL; an
 * unknown format: MDC_EINVAL.
 *
 * mdc_iq_windows_norm: sum_i, sum_q, sum_sq and the energy E are defined on s exactly as in the block above
 * (E = 128*sum_sq - sum_i^2 - sum_q^2 with MDC_IQ_REMOVE_DC, 128*sum_sq without) and returned as exact integers in the
 * 32-byte record below.  Bounds:   |sum_i|, |sum_q|      sum_sq            E
 *     MDC_IQ_CU8                   <= 32,640             <= 16,646,400     <= 2,130,739,200 (the four values of mdc_iq_window_stats)
 *     MDC_IQ_CI8                   <= 2^14               <= 2^22           <= 2^29
 *     MDC_IQ_CI16                  <= 2^22               <= 2^38           <= 2^45
 * Frames, normatively, are the chain of operations of mdc_iq_u8_windows_norm:
 *     x = (float)(128*s - c) * (level / sqrtf((float)E)),   c = the channel's sum under MDC_IQ_REMOVE_DC, else 0;
 * |128*s - c| < 2^24 in every format, so its conversion is exact; (float)E is ONE correctly rounded conversion of the 64-bit
 * integer; square root, division and multiplication are correctly rounded: |x - exact| <= 2^-21 |exact| as above.  E == 0
 * gives an all-zero frame.  (MDC_IQ_CI16 with a level so small that level / sqrt(E) nears the f32 denormals -- 1e-30 -- is
 * outside this bound.)  With MDC_IQ_CU8 the frames are bit-identical to mdc_iq_u8_windows / mdc_iq_u8_windows_norm.
 * The window's power relative to a full-scale constant-envelope one is E / (128*A)^2 (10*log10 of it: dBFS); the largest
 * possible window is +3 dB in every format.
 * x_dev (n,2,128) f32, 8-byte aligned; stats64_dev (n), 16-byte aligned; in mdc_iq_windows_norm each may be NULL, not both.
 * level, flags as mdc_iq_u8_windows_norm.  n == 0 is MDC_OK.  Both calls only enqueue on hip_stream (no synchronisation, no
 * allocation: capturable in a hipGraph) and run on the current device.
 * Float captures (cf32) are no fourth format of these entries: mdc_iq_cf32_quantize, below, turns one into an MDC_IQ_CI16 stream
 * once, in front of them.  Big-endian 16-bit samples must be swapped by the caller. */
enum { MDC_IQ_CU8 = 0, MDC_IQ_CI8 = 1, MDC_IQ_CI16 = 2 };

typedef struct mdc_iq_window_stats64 {   /* 32 B */
    int64_t  sum_i, sum_q;
    uint64_t sum_sq;
    uint64_t energy;
} mdc_iq_window_stats64;

MDC_API int mdc_iq_windows(const void* iq_dev, int format, int64_t n, int64_t hop, float scale, float* x_dev, void* hip_stream);
MDC_API int mdc_iq_windows_norm(const void* iq_dev, int format, int64_t n, int64_t hop, float level, int flags,
                           float* x_dev, mdc_iq_window_stats64* stats64_dev, void* hip_stream);

/* ---- float captures: exponent histogram and exact quantiser of complex float32 into MDC_IQ_CI16 (additive in ABI 5) ------------
 * GNU Radio's file sink, UHD's fc32 and SigMF's cf32_le write interleaved complex float32.  Such a capture is converted ONCE, at
 * the door, into an ordinary MDC_IQ_CI16 stream: everything behind it stays exact-integer and bit-reproducible.  Two decisions
 * make that conversion as well defined as the integer entries (the numpy restatement is tests/iq_cf32_ref.py):
 *   input       iq_dev holds 2 * pairs_in little-endian IEEE-754 binary32 values, I0 Q0 I1 Q1 ..., aligned to ONE PAIR (8 bytes)
 *               and to nothing more: a buffer that starts 8 bytes off a 16-byte boundary is served.
 *   histogram   the "exact statistics" of a float capture are integer counts: for every component with bit pattern b,
 *               hist[(b >> 23) & 0xFF] += 1, the biased exponent byte.  Bin 0 holds zeros and denormals; bin e in 1 .. 254 the
 *               normal numbers with 2^(e-127) <= |x| < 2^(e-126); bin 255 NaN and +-Inf.  The bins sum to 2 * pairs_in.  The call
 *               ADDS into hist_dev (256 uint64, 8-byte aligned): the caller zeroes it, and a file read in chunks accumulates.
 *               Counts are order-free: bit-identical on every run.  They answer "which power-of-two gain?" on the host, also
 *               for a capture with a few glitch samples that a plain maximum would be ruined by (the library's Python mirror
 *               has the design: frontend.design_cf32_gain).
 *   quantiser   gain must be a finite f32 in [2^-126, 2^125], else MDC_EINVAL.  Per pair: if either component is non-finite
 *               (exponent byte 255) the pair becomes (0, 0) and counts[0] += 1.  Otherwise, per component: t = x * gain as ONE
 *               correctly rounded f32 multiplication; r = rintf(t), to nearest, ties to even; if r > 32767 or r < -32768,
 *               counts[1] += 1; the output is clamp(r, -32768, 32767) as int16.  A finite x whose product overflows to +-Inf is
 *               clipped and counted, not treated as non-finite.  With a power-of-two gain the multiplication is exact and the
 *               quantisation is one rounding per sample.  In the gain's range a denormal x times the gain is below 2^-126 *
 *               2^125 = 0.5 in magnitude and rounds to 0, as a denormal flushed to zero does -- and a product that is itself
 *               denormal rounds to 0 either way: the result does not depend on whether denormals are flushed.
 *               counts_dev (2 uint64, 8-byte aligned: non-finite pairs, clipped components) is ADDED to and may be NULL.
 *   output      pairs_in int16 pairs, out_dev 4-byte aligned, not overlapping the input.  The pass is pointwise: a capture
 *               converted in pieces gives the same bits as in one call.
 * pairs_in <= 2^40 per call (the work-groups count in 32 bits), otherwise MDC_EINVAL.  Every argument error is MDC_EINVAL with a
 * mdc_last_error() text before any device call; pairs_in == 0 is MDC_OK with nothing launched.  Both calls only enqueue on
 * hip_stream (no synchronisation, no allocation, no memset: capturable in a hipGraph) and run on the current device.
 * 0 dBFS of everything computed from the result is the float amplitude 32768 / gain.  A 16-bit stream carries 16 bits: an
 * emitter more than about 80 dB below the capture's peak is lost to the rounding. */
MDC_API int mdc_iq_cf32_histogram(const float* iq_dev, int64_t pairs_in, uint64_t* hist_dev /* 256 */, void* hip_stream);
MDC_API int mdc_iq_cf32_quantize(const float* iq_dev, int64_t pairs_in, float gain, int16_t* out_dev,
                           uint64_t* counts_dev /* 2, may be NULL */, void* hip_stream);

/* ---- I/Q balance: a receiver's gain / phase imbalance and DC offset, measured and corrected (additive in ABI 5) -----------------
 * A zero-IF receiver's I and Q rails differ in gain by a fraction of a dB to a dB and are a few degrees off 90: every emitter
 * at +f then has a mirror image at -f, 20 .. 40 dB below it (1 dB and 5 degrees: 22.83 dB), which a detector 6 dB above the
 * floor reports as an emitter of its own.  mdc_iq_balance_stats measures, the caller designs six integers on the host, and
 * mdc_iq_balance applies them: all in EXACT integer arithmetic (the numpy int64 restatement is tests/iq_balance_ref.py), the
 * result an ordinary MDC_IQ_CI16 stream for every other mdc_iq_* entry.  Normatively, with (x_n, y_n) the widened I and Q of
 * input pair n -- the widening is mdc_iq_ddc's, below --:
 *   statistics  the capture is cut into blocks of B = block_pairs pairs, 64 <= B <= 2^20, ANY integer in between (an odd B puts
 *               blocks on odd pairs); block b covers the pairs [b B, min((b + 1) B, pairs_in)), the last one may be partial:
 *               nblocks = ceil(pairs_in / B) = mdc_iq_balance_blocks.  Per block five int64 sums, in this order:
 *               sum x, sum y, sum x^2, sum y^2, sum x y; sums_dev is nblocks x 5, block-major.  |sum x^2| <= 2^20 * 2^30:
 *               every sum is exact, so any order of summation gives the same bits.  The whole capture's sums are the blocks'
 *               sums added on the host; a caller may leave blocks out (a stretch where a strong real-valued emitter sits on
 *               0 Hz), or compare blocks to see the imbalance drift.
 *   design      (host; the library's Python mirror has one: frontend.design_balance) dc = the means of x and y, rounded;
 *               M = sqrt(tr C / 2) C^(-1/2), C the covariance of (x, y): the symmetric whitening matrix, which equalises the
 *               rails, makes them orthogonal, keeps the total power and does not rotate; m_ij = rint(16384 M_ij), Q14.
 *   correction  a = x - dc_i, b = y - dc_q;
 *               out_I = clamp((m00 a + m01 b + 8192) >> 14, -32768, 32767), out_Q likewise with m10, m11 (arithmetic
 *               shift: round half up).  Hard preconditions: |dc_i|, |dc_q| <= 32768 and |m_i0| + |m_i1| <= 32767 per row.
 *               Then |a|, |b| <= 32768 + 32768 = 65536, |m_i0 a + m_i1 b| <= 32767 * 65536 = 2^31 - 65536, and + 8192 stays
 *               below 2^31: 32-bit accumulation is exact.  The identity is (0, 0, 16384, 0, 0, 16384): MDC_IQ_CI16 comes out
 *               as it went in, the 8-bit formats come out widened.  A general matrix also expresses the I/Q swap of a
 *               wrongly wired capture (spectrum inversion), (0, 16384, 16384, 0), and conjugation, (16384, 0, 0, -16384).
 *   output      pairs_in int16 pairs.  The pass is pointwise: a capture corrected in pieces gives the same bits as in one call.
 * The estimate is BLIND: it takes the capture as a whole to be proper, E[z^2] = 0.  Any mix of emitters away from 0 Hz and
 * from half the rate is (a BPSK at f0 turns at 2 f0 and averages out); a dominant real-valued modulation (BPSK, PAM, AM-DSB)
 * centred exactly on 0 Hz is not, and is taken for imbalance: leave its blocks out, or pass coefficients measured elsewhere.
 * The imbalance is taken as flat over the band: one matrix, no frequency dependence.
 * iq_dev is aligned to one pair (2 / 2 / 4 bytes), sums_dev to 8 bytes, out_dev to 4 bytes; out_dev must not overlap the input.
 * coeffs_host is read (and validated) during the call and travels with the launch.  nblocks must equal
 * mdc_iq_balance_blocks.  Every argument error is MDC_EINVAL before any device call; pairs_in == 0 is MDC_OK with nothing
 * launched.  Both calls only enqueue on hip_stream (no synchronisation, no allocation: capturable in a hipGraph) and run on
 * the current device.  mdc_iq_balance_blocks returns nblocks, or a negative MDC_EINVAL. */
typedef struct mdc_iq_balance_coeffs {   /* 24 B */
    int32_t dc_i, dc_q;             /* subtracted from the widened I and Q */
    int32_t m00, m01, m10, m11;     /* Q14 */
} mdc_iq_balance_coeffs;
MDC_API int64_t mdc_iq_balance_blocks(int64_t pairs_in, int64_t block_pairs);
MDC_API int mdc_iq_balance_stats(const void* iq_dev, int format, int64_t pairs_in, int64_t block_pairs,
                           int64_t* sums_dev /* nblocks x 5 */, int64_t nblocks, void* hip_stream);
MDC_API int mdc_iq_balance(const void* iq_dev, int format, int64_t pairs_in, const mdc_iq_balance_coeffs* coeffs_host,
                           int16_t* out_dev, void* hip_stream);

/* ---- digital down-converter: frequency shift, low-pass, decimate (additive in ABI 5) ---------------------------------------
 * A capture comes off the radio at its own rate and with the signal at some offset from the tuner's centre; the nets want
 * 8 samples per symbol at 0 Hz.  mdc_iq_ddc does what lies between, on the device, in EXACT integer arithmetic: the output is
 * the same bits on every machine (the numpy int64 restatement is tests/iq_ddc_ref.py) and is an ordinary MDC_IQ_CI16 stream
 * for mdc_iq_windows / mdc_iq_windows_norm.  Normatively, for the pairs_in input pairs (I_n, Q_n), n counted from iq_dev:
 *   widening   to 16-bit full scale: MDC_IQ_CU8 (2*byte - 255)*128, MDC_IQ_CI8 s*256, MDC_IQ_CI16 s  (|.| <= 32768; 0 dBFS
 *              stays 0 dBFS)
 *   oscillator phi_n = (phase0 + n*phase_step) mod 2^32; k = phi_n >> 20 indexes a table of 4096 int16 pairs
 *              c_k = rint(32767 cos(2 pi k / 4096)), s_k = rint(32767 sin(2 pi k / 4096))  (the table itself:
 *              mdc_iq_ddc_nco_table).  The mixer multiplies by e^{+j 2 pi phi / 2^32}: phase_step / 2^32 cycles per sample are
 *              ADDED to every component; a signal at +f0 comes to 0 with a step of -f0.  The 12-bit table's spurs lie near
 *              -72 dBc.
 *   mixer      m_re = (I c - Q s + 32768) >> 16,  m_im = (I s + Q c + 32768) >> 16  (arithmetic shifts: round half up).
 *              |I c - Q s| <= 2 * 32768 * 32767, + 32768 < 2^31; |m| <= 32767: an int16 holding HALF the product.
 *   filter     taps h_0 .. h_{T-1}: int16, Q15 (DC gain 1 is a sum of 32768), applied as written (no reversal), with the hard
 *              precondition sum |h_k| <= 65535.  Output j: acc = sum_k h_k m_{jD+k}, re and im separately;
 *              |acc| <= 32767 * 65535, + 8192 < 2^31: 32-bit accumulation is exact.
 *              out = clamp((acc + 8192) >> 14, -32768, 32767): the shift restores the mixer's halving.
 *   output     n_out = pairs_in >= T ? (pairs_in - T) / D + 1 : 0 int16 pairs: a "valid" convolution, no invented edge
 *              samples.  The filter's group delay, (T-1)/2 input pairs for symmetric taps, is not compensated.
 * 1 <= decimate D <= 256, 1 <= ntaps T <= 1024.  A capture processed in pieces gives the same bits as in one call when piece
 * two starts at input pair a = (a multiple of D) with phase0 + a*phase_step and the pieces overlap by T - D pairs.
 * taps_host is read (and validated) during the call and travels with the launch: it may be freed on return, and nothing is
 * copied that would need a synchronisation.  iq_dev is aligned to one pair (2 / 2 / 4 bytes), out_dev to 4 bytes; n_out must
 * equal mdc_iq_ddc_out_count.  Every argument error is MDC_EINVAL before any device call.  n_out == 0 is MDC_OK.  The call only
 * enqueues on hip_stream (no synchronisation, no allocation: capturable in a hipGraph) and runs on the current device.
 * mdc_iq_ddc_out_count returns n_out, or a negative MDC_EINVAL; mdc_iq_ddc_nco_table writes the 4096 (cos, sin) pairs and
 * needs no device. */
MDC_API int64_t mdc_iq_ddc_out_count(int64_t pairs_in, int ntaps, int decimate);
MDC_API int mdc_iq_ddc_nco_table(int16_t* cos_sin_host /* 4096 x 2 */);
MDC_API int mdc_iq_ddc(const void* iq_dev, int format, int64_t pairs_in, uint32_t phase0, uint32_t phase_step, int decimate,
                       const int16_t* taps_host, int ntaps, int16_t* out_dev, int64_t n_out, void* hip_stream);

/* ---- rational resampler: frequency shift, low-pass, resample by L/D (additive in ABI 5) ------------------------------------
 * Integer decimation reaches the nets' 8 samples per symbol only when the radio's rate is an integer multiple of 8 x the symbol
 * rate (2.4 MS/s on 250 ksym/s is 9.6 samples per symbol: 5/6 gives 8).  mdc_iq_resample is mdc_iq_ddc with an interpolation
 * factor L = interpolate in front of the filter, in the same EXACT integer arithmetic (the numpy int64 restatement is
 * tests/iq_resample_ref.py).  Normatively, for the pairs_in = P input pairs:
 *   widening, oscillator, mixer   word for word those of mdc_iq_ddc: m_n (int16, half the product), n = 0 .. P-1; the
 *              oscillator advances once per INPUT pair.
 *   zero stuffing   v has length Lv = (P-1) L + 1; v_{nL} = m_n, every other v is 0.  No zeros are invented after the last
 *              sample.
 *   filter     prototype taps h_0 .. h_{T-1}: int16, at the INTERPOLATED rate, applied as written.  Output j:
 *              acc_j = sum_k h_k v_{jD+k}, re and im separately.  Only k = r_j (mod L) contribute, r_j = (-jD) mod L, so
 *              acc_j = sum_i h_{r_j + iL} m_{ceil(jD/L) + i}: output j uses branch r_j of the polyphase decomposition.  A branch
 *              without taps (possible when T < L) gives 0.
 *              Hard precondition: for EVERY branch r, sum_i |h_{r+iL}| <= 65535 (the prototype's sum may be up to L times
 *              that).  Then |acc| <= 32767 * 65535, + 8192 < 2^31: 32-bit accumulation is exact.  DC gain 1 means every branch
 *              sums to 32768 (the prototype to 32768 L).
 *              out = clamp((acc + 8192) >> 14, -32768, 32767), as in mdc_iq_ddc.
 *   output     n_out = (P >= 1 && Lv >= T) ? (Lv - T) / D + 1 : 0 int16 pairs.
 * 1 <= interpolate L <= 32, 1 <= decimate D <= 256, 1 <= ntaps T <= 1024, pairs_in <= 2^58; gcd(L, D) need not be 1.  L = 1 is
 * exactly mdc_iq_ddc: the same bits for the same arguments.  Pieces: the outputs of a prefix of the capture are a prefix of the
 * outputs; a call on the pairs from a on, with a L = 0 (mod D) and phase0 + a*phase_step, returns the whole call's outputs from
 * j0 = a L / D on.  Alignment, null and n_out conventions are mdc_iq_ddc's: taps_host is read and validated during the call and
 * travels with the launch (it may be freed on return); iq_dev is aligned to one pair, out_dev to 4 bytes; n_out must equal
 * mdc_iq_resample_out_count.  Every argument error is MDC_EINVAL before any device call -- a branch over 65535 names the branch
 * and its sum.  n_out == 0 is MDC_OK.  The call only enqueues on hip_stream (no synchronisation, no allocation: capturable in a
 * hipGraph) and runs on the current device.  mdc_iq_resample_out_count returns n_out, or a negative MDC_EINVAL. */
MDC_API int64_t mdc_iq_resample_out_count(int64_t pairs_in, int ntaps, int interpolate, int decimate);
MDC_API int mdc_iq_resample(const void* iq_dev, int format, int64_t pairs_in, uint32_t phase0, uint32_t phase_step, int interpolate,
                            int decimate, const int16_t* taps_host, int ntaps, int16_t* out_dev, int64_t n_out, void* hip_stream);

/* ---- batched extraction: K stretches of one capture, each tuned, filtered and resampled, in one launch (additive in ABI 5) ----
 * A search over a capture (mdc_iq_spectrogram_components) returns hundreds to thousands of boxes; K calls of mdc_iq_resample on
 * K slices are K launches, each with its taps.  mdc_iq_extract does all of them in one: a JOB is a stretch of the capture with
 * its own oscillator and filter, and its outputs go to a range of one output buffer.  Normatively, for job j of the plan:
 *     out_dev[out_first .. out_first + n_out)  =  the first n_out output pairs of
 *     mdc_iq_resample(iq_dev + first_pair pairs, format, pairs, phase0, phase_step, L, D, taps, ...)
 * bit for bit, (L, D, taps) being filters[job.filter]: the oscillator counts from the job's own first pair, and pairs at or
 * beyond first_pair + pairs read as zero even where the capture goes on -- the semantics of a call on the slice.  For L = 1 it
 * is mdc_iq_ddc's result.  0 <= n_out <= mdc_iq_resample_out_count(pairs, ntaps, L, D): a caller may trim each job, to whole
 * frames of 128 pairs for instance, and pack the jobs back to back.  Pairs of out_dev that no job names are not written.
 *   filters    filters_host[f] = (interpolate, decimate, ntaps, first_tap): the filter's taps are taps_host[first_tap ..
 *              first_tap + ntaps), int16, under mdc_iq_resample's limits (L <= 32, D <= 256, T <= 1024, per branch
 *              sum |h| <= 65535).  Filters may share or overlap stretches of taps_host.
 *   jobs       jobs_host[j]: 0 <= first_pair, 0 <= pairs, first_pair + pairs <= pairs_in; 0 <= filter < nfilters; reserved = 0;
 *              the output ranges [out_first, out_first + n_out) lie inside [0, out_pairs] and are pairwise disjoint (ranges that
 *              merely touch are disjoint; empty ranges overlap nothing).  Jobs may read overlapping input.
 *   plan       mdc_iq_extract_plan validates all of that and writes a position-independent blob of exactly
 *              mdc_iq_extract_plan_bytes(...) bytes into plan_host: a header, the job records, per filter the tiling and the
 *              branch-major tap image the kernel reads, and the list of (job, tile) work items, ordered so that the tiles of one
 *              filter are adjacent.  Both calls are host code and need no device; the same inputs give the same bytes.
 *              mdc_iq_extract_plan_bytes checks what it can see (the filters' limits, each job's filter index, reserved, pairs
 *              and n_out) and returns the size, or a negative MDC_EINVAL.  Every failure is MDC_EINVAL with a message that names
 *              the job (or the filter).
 *   run        the caller moves the blob to the device as it likes (plan_dev: the same plan_bytes bytes, 8-byte aligned) and
 *              calls mdc_iq_extract with BOTH copies: launch sizes and the sanity checks (magic, size, and that format, pairs_in
 *              and out_pairs are the plan's) come from plan_host, the kernel reads plan_dev.  The call only enqueues on
 *              hip_stream -- no allocation, no copy, no synchronisation: capturable in a hipGraph -- and runs on the current
 *              device; plan_host may be freed on return, plan_dev must live until the launch has run.  A plan without tiles is
 *              MDC_OK without a launch.  iq_dev is aligned to one pair, out_dev to 4 bytes, as in mdc_iq_resample.
 * A plan may be run any number of times, on any capture of the same format and length. */
typedef struct mdc_iq_extract_filter {
    int32_t interpolate, decimate, ntaps;
    int32_t first_tap;                   /* index of the filter's first tap in taps_host */
} mdc_iq_extract_filter;
typedef struct mdc_iq_extract_job {
    int64_t first_pair, pairs;           /* the stretch [first_pair, first_pair + pairs) of the capture */
    int64_t out_first, n_out;            /* its outputs: pairs [out_first, out_first + n_out) of out_dev */
    uint32_t phase0, phase_step;         /* the oscillator, counted from first_pair */
    int32_t filter, reserved;            /* index into filters_host; 0 */
} mdc_iq_extract_job;
MDC_API int64_t mdc_iq_extract_plan_bytes(int64_t njobs, int32_t nfilters, const mdc_iq_extract_job* jobs_host,
                                          const mdc_iq_extract_filter* filters_host);
MDC_API int mdc_iq_extract_plan(int format, int64_t pairs_in, const mdc_iq_extract_job* jobs_host, int64_t njobs,
                                const mdc_iq_extract_filter* filters_host, int32_t nfilters, const int16_t* taps_host, int64_t ntaps_total,
                                int64_t out_pairs, void* plan_host, int64_t plan_bytes);
MDC_API int mdc_iq_extract(const void* iq_dev, int format, int64_t pairs_in, const void* plan_host, const void* plan_dev, int64_t plan_bytes,
                           int16_t* out_dev, int64_t out_pairs, void* hip_stream);

/* ---- power spectrogram: windowed FFTs of a raw capture, averaged (additive in ABI 5) ----------------------------------------
 * mdc_iq_ddc and mdc_iq_resample want to be told where the signal is and how wide; mdc_iq_spectrogram is what finds out: the
 * power spectrum of the capture, segment by segment, on the device (the float64 numpy restatement is tests/iq_spectrum_ref.py).
 * Normatively, for the pairs_in = P input pairs x_n = (I_n, Q_n), n counted from iq_dev:
 *   widening   to 16-bit full scale, as in mdc_iq_ddc: MDC_IQ_CU8 (2*byte - 255)*128, MDC_IQ_CI8 s*256, MDC_IQ_CI16 s.
 *   segments   segment s starts at pair s*hop and holds nfft pairs; segs = P >= nfft ? (P - nfft) / hop + 1 : 0.  hop < nfft
 *              (overlap), hop == nfft and hop > nfft (a sparse, fast scan that skips pairs) are all legal.
 *   window     v_s[n] = x[s*hop + n] * w[n], n = 0 .. nfft-1, w the nfft int16 values at window_dev (a DEVICE buffer: 8 KiB do
 *              not travel with a launch the way taps do), applied as written.  Both components are exact integers, |v| < 2^30.
 *   spectrum   X_s[k] = sum_n v_s[n] e^{-2 pi i k n / nfft}, k = 0 .. nfft-1.
 *   rows       rows = segs / avg; row r averages segments r*avg .. r*avg + avg-1:
 *              P[r,k] = scale * (1/avg) * sum_s |X_s[k]|^2, float32, in natural DFT order (bin k is k/nfft cycles per sample,
 *              k >= nfft/2 the negative frequencies), rows contiguous: power_dev holds rows * nfft floats.  Trailing segments
 *              that do not fill a row are DROPPED.
 * The transform runs in float32 (twiddle factors rounded from float64), the segments of a row are summed in a fixed order by
 * one work-group: the same inputs give the same bits on every run, and row r of a call equals, bit for bit, the single row of a
 * call on the pairs from r*avg*hop on.  With u = 2^-24 and eps = 8u (log2 nfft + 1) every value lies within
 * mean_s[2 eps sqrt(P_s[k] T_s) + eps^2 T_s] + (avg + 4) u P[r,k] of the definition (P_s: one segment's scaled power, T_s its
 * sum over the bins).
 * nfft: a power of two in 64..4096; hop >= 1; 1 <= avg <= 4096; scale finite and > 0; rows must equal
 * mdc_iq_spectrogram_rows.  iq_dev is aligned to one pair (2 / 2 / 4 bytes), window_dev to 2 bytes, power_dev to 4 bytes.  Every
 * argument error is MDC_EINVAL before any device call.  rows == 0 is MDC_OK (nothing is launched; the buffers may be NULL); otherwise no
 * buffer may be NULL.  The call only enqueues on hip_stream (no synchronisation, no allocation, no copy: capturable in a
 * hipGraph) and runs on the current device.  mdc_iq_spectrogram_rows returns rows, or a negative MDC_EINVAL. */
MDC_API int64_t mdc_iq_spectrogram_rows(int64_t pairs_in, int nfft, int64_t hop, int avg);
MDC_API int mdc_iq_spectrogram(const void* iq_dev, int format, int64_t pairs_in, int nfft, int64_t hop, int avg,
                               const int16_t* window_dev, float scale, float* power_dev, int64_t rows, void* hip_stream);

/* ---- line spectrum: the power spectrogram of a pointwise power of the capture (additive in ABI 5) ---------------------------
 * A pulse-shaped linear modulation hides two spectral lines: the spectrum of |x|^2 has one at the symbol rate, and the spectrum
 * of x^2 (BPSK, PAM) or x^4 (QPSK, QAM) one at 2 or 4 times the residual carrier offset.  mdc_iq_line_spectrum is
 * mdc_iq_spectrogram with one more step between widening and window (the float64 numpy restatement is tests/iq_line_ref.py).
 * Normatively, with (I, Q) the pair widened to 16-bit full scale, y_n is the exact integer pair
 *   order 0    MDC_IQ_LINE_ENVELOPE: y = (I^2 + Q^2, 0), |y| <= 2^31;
 *   order 1    y = (I, Q): the result is mdc_iq_spectrogram's, bit for bit;
 *   order 2    y = (I^2 - Q^2, 2 I Q), the square of I + iQ; both components within +-2^31 (I = Q = -32768 reaches 2^31);
 *   order 4    y = (a^2 - b^2, 2 a b), (a, b) the order-2 pair: the fourth power, both components within +-2^62;
 * any other order is MDC_EINVAL.  The staged value is
 *   window     v_s[n] = y[s*hop + n] * w[n] * 2^-q,  q = 16 for orders 0 and 2, 48 for order 4, 0 for order 1:  |v| <= 2^30,
 *              so that |X|^2 summed over avg <= 4096 segments stays inside float32 at every order.
 * Segments, spectrum, rows, averaging and scale are the power spectrogram's, with v_s as above; so are the output order, the
 * dropped trailing segments, the limits on nfft, hop, avg and scale, the alignment and NULL rules, rows == 0, "only enqueues",
 * graph capture and both determinism statements (the same bits on every run; row r equals the one-row call on the pairs from
 * r*avg*hop on).  rows must equal mdc_iq_spectrogram_rows(pairs_in, nfft, hop, avg): there is no second counting function.
 * Error bound: the power spectrogram's formula with eps = u (8 (log2 nfft + 1) + c), c = 2 for orders 0, 2 and 4 (c = 0 for
 * order 1, whose integers convert exactly).  c counts the float32 roundings on a value before the transform: y is formed in
 * integers (32-bit for orders 0 and 2, 64-bit for order 4) and is exact; its conversion to float32 rounds once (|y| is no longer
 * below 2^24); w[n] * 2^-q is an int16 times a power of two, exact (the factor 2 of 2 I Q and of 2 a b is folded into it or into
 * the integer, exactly); the product of the two rounds once more.  No value is subnormal: |y w| >= 1 or 0, and 2^-48 is far
 * from float32's smallest normal.  By Parseval a relative perturbation c u of every v moves every bin of X_s by at most
 * c u sqrt(T_s / scale), which is the form the bound already has. */
#define MDC_IQ_LINE_ENVELOPE 0
MDC_API int mdc_iq_line_spectrum(const void* iq_dev, int format, int64_t pairs_in, int order, int nfft, int64_t hop, int avg,
                                 const int16_t* window_dev, float scale, float* power_dev, int64_t rows, void* hip_stream);

/* ---- batched line spectra: the line spectra of K stretches, and their means, in one call (additive in ABI 5) ----------------
 * A search returns hundreds of boxes, and each box's symbol rate and carrier offset are read from the lines of its own isolated
 * stream (mdc_iq_extract puts all of those streams into one MDC_IQ_CI16 block).  One mdc_iq_line_spectrum per (box, order) is
 * three launches per box; mdc_iq_line_spectra does all boxes and all orders in one call.  A JOB is a stretch
 * [first_pair, first_pair + pairs) of the capture at iq_dev; jobs may overlap, be empty, and start on any pair.
 *   rows fn    mdc_iq_line_spectra_rows (host code, no device) checks 0 <= first_pair, 0 <= pairs, first_pair + pairs <= pairs_in
 *              for every job and FILLS each job's rows = mdc_iq_spectrogram_rows(pairs, nfft, hop, avg) and first_row, the sum of
 *              the rows of the jobs before it; it returns the total number of rows, or a negative MDC_EINVAL whose message names
 *              the job.
 *   rows       rows_dev holds norders planes of total_rows rows of nfft floats: [order index][global row][nfft].  For job j and
 *              orders_host[i] = o, rows first_row .. first_row + rows - 1 of plane i equal, bit for bit, what
 *              mdc_iq_line_spectrum(iq_dev + first_pair pairs, format, pairs, o, nfft, hop, avg, window_dev, scale, ...) writes
 *              (the same kernel computes them).  No pair outside the job is read.
 *   means      mean_dev holds njobs * norders * nfft doubles, [job][order index][nfft]: mean_dev[j][i][k] is
 *              acc = 0.0; for r = first_row .. first_row + rows - 1 in that order: acc += (double)row[r][k]; acc / (double)rows
 *              in IEEE float64 -- the bits of that loop.  A job with rows == 0 gets 0.0 in all its bins.
 *   orders     orders_host: 1 <= norders <= 4 DISTINCT values of 0 (MDC_IQ_LINE_ENVELOPE), 1, 2, 4, in any order; a HOST array
 *              that travels with the launch.
 *   launches   norders + 1 per call, at most five, however many jobs there are -- mdc_iq_line_spectrum's own kernel once per order
 *              over all jobs' rows, then the means -- on hip_stream; the row launches are skipped when total_rows == 0, all
 *              when njobs == 0.  Work-groups look their row's job up in the table; the grid is capped and strides.  No work-group waits for another, nothing is atomic: the same inputs give the same bits on every run,
 *              and a job's rows and means depend on neither the other jobs nor their order.
 * The caller passes the job table twice, as mdc_iq_extract takes its plan: launch sizes and every check come from jobs_host
 * (whose first_row / rows must be what mdc_iq_line_spectra_rows fills, and total_rows what it returns), the kernels read jobs_dev,
 * the same njobs records on the device, 8-byte aligned; jobs_host may be freed on return.  The limits on nfft, hop, avg and scale
 * and the alignment of iq_dev, window_dev and rows_dev are mdc_iq_line_spectrum's; mean_dev is 8-byte aligned.  Every argument
 * error is MDC_EINVAL with a message, before any device call.  The call only enqueues (no allocation, no copy, no
 * synchronisation: capturable in a hipGraph) and runs on the current device.  njobs <= 2^24. */
typedef struct mdc_iq_line_job {
    int64_t first_pair, pairs;           /* the stretch [first_pair, first_pair + pairs) of the capture */
    int64_t first_row, rows;             /* its rows in every plane of rows_dev: filled by mdc_iq_line_spectra_rows */
} mdc_iq_line_job;
MDC_API int64_t mdc_iq_line_spectra_rows(mdc_iq_line_job* jobs_host, int64_t njobs, int64_t pairs_in, int nfft, int64_t hop, int avg);
MDC_API int mdc_iq_line_spectra(const void* iq_dev, int format, int64_t pairs_in, const mdc_iq_line_job* jobs_host,
                                const mdc_iq_line_job* jobs_dev, int64_t njobs, const int* orders_host, int norders, int nfft, int64_t hop,
                                int avg, const int16_t* window_dev, float scale, float* rows_dev, int64_t total_rows, double* mean_dev,
                                void* hip_stream);

/* ---- line search: the strongest line of S power spectra within a band each, on the device (additive in ABI 5) ----------------
 * What a host does with a line spectrum -- an argmax inside a band, the band's median, the peak's two neighbours -- needs the
 * whole spectrum on the host: nfft doubles per spectrum.  mdc_iq_find_lines does the search where the spectra are and leaves
 * one record of 48 bytes per spectrum.  Normatively, for spectrum s, the nfft doubles at spectra_dev + s * nfft in natural DFT
 * order (what mdc_iq_line_spectra writes to mean_dev), and its band (lo, hi, two_sided):
 *   searched   the bins k with lo <= g <= hi, g = f or, when two_sided != 0, |f|;  f = k / nfft for k < nfft / 2, else
 *              (k - nfft) / nfft, formed and compared in float64.
 *   count      the number of searched bins.
 *   bin        the searched bin that holds the largest value; among equal values the smallest k.
 *   peak       that value; left and right are the values of bins k - 1 and k + 1 modulo nfft, searched or not.
 *   medians    median_lo and median_hi are the order statistics (count - 1) / 2 and count / 2 (0-based, integer division) of the
 *              searched values sorted ascending: equal for an odd count; their mean is the median.
 * All five doubles are elements of the spectrum, bit for bit.  A spectrum that holds, in any bin, a NaN, an infinity or a value
 * below zero gets count = -1 and the other fields are unspecified (-0.0 counts as zero).  A band without a bin is MDC_EINVAL, found on the
 * host from bands_host before any device call, with a message that names the spectrum; reserved must be 0.  bands_host is
 * read for the checks, the kernel reads bands_dev (the same records on the device); all three device buffers are 8-byte
 * aligned.  nfft: a power of two in 64..4096.  nspectra == 0 is MDC_OK without a launch.  One launch, one work-group per
 * spectrum (the grid is capped and strides); the call only enqueues and is capturable in a hipGraph. */
typedef struct mdc_iq_line_band {
    double lo, hi;                       /* cycles per sample */
    int32_t two_sided, reserved;         /* != 0: the band is on |f|; 0 */
} mdc_iq_line_band;
typedef struct mdc_iq_line_record {
    int32_t bin, count;
    double peak, left, right, median_lo, median_hi;
} mdc_iq_line_record;
MDC_API int mdc_iq_find_lines(const double* spectra_dev, int64_t nspectra, int nfft, const mdc_iq_line_band* bands_host,
                              const mdc_iq_line_band* bands_dev, mdc_iq_line_record* records_dev, void* hip_stream);

/* ---- spectrum quantiles: per-bin order statistics of a spectrogram along time (additive in ABI 5) ---------------------------
 * The mean over a spectrogram's rows dilutes an emitter that is on for 3 % of the capture by 15 dB.  A high quantile over time
 * per bin ("the level this bin reaches in its top 2 % of rows") shows it at full strength and, unlike max-hold, shrugs off single
 * noisy rows; the median over time is a noise floor that bursts do not lift.  mdc_iq_spectrum_quantiles computes up to 8 such
 * order statistics of every column in one call (the numpy restatement is tests/iq_quantile_ref.py).
 * Normatively, for power_dev = rows * nfft floats, rows contiguous (what mdc_iq_spectrogram / mdc_iq_line_spectrum write):
 *   order      for every column k, the `rows` 32-bit patterns power_dev[r*nfft + k] are sorted ascending AS UNSIGNED INTEGERS;
 *   result     out_dev[i*nfft + k] is the pattern at position ranks_host[i] (0-based) of that order: out_dev holds
 *              nranks * nfft floats, rank-major.
 * For finite non-negative floats, +0, subnormals and +Inf that order is the numeric one, and the spectrogram produces nothing
 * else.  A pattern with the sign bit set, or a NaN, is ordered by the same rule -- after every non-negative float, -0 before
 * the other negative values, those by growing magnitude -- which is defined and memory-safe, if of no numeric use.  The result
 * is an element of the column: nothing is interpolated, so it is the same bits on every run and on every machine, and column
 * k's result depends on no other column.
 * 1 <= rows <= 2^31 - 1; nfft: a power of two in 64..4096; 0 <= nranks <= 8; every rank in 0 .. rows-1, in any order, repeats
 * allowed.  ranks_host is a HOST array, read and validated during the call: the ranks travel with the launch (as mdc_iq_ddc's
 * taps do) and the array may be freed on return.  power_dev and out_dev are 4-byte aligned.  nranks == 0 is MDC_OK (nothing is
 * launched; the buffers may be NULL); otherwise no buffer may be NULL.  Every argument error is MDC_EINVAL before any device
 * call.  The call only enqueues on hip_stream (no synchronisation, no allocation, no copy: capturable in a hipGraph) and runs
 * on the current device. */
MDC_API int mdc_iq_spectrum_quantiles(const float* power_dev, int64_t rows, int nfft, const int64_t* ranks_host, int nranks,
                                      float* out_dev, void* hip_stream);

/* ---- spectrogram components: a time-frequency detector on a thresholded spectrogram (additive in ABI 5) ----------------------
 * A frequency hopper never dwells in one bin long enough to show in a quantile spectrum, two intermittent emitters that share
 * bins at different times come out of it as one, and a single short packet is below any quantile the rows allow.  All three are
 * plain to see in two dimensions: threshold the spectrogram cell by cell, join neighbouring on-cells into connected components,
 * and reduce each component to a box in time and frequency.  mdc_iq_spectrogram_components does that on the device in one call
 * (the Python restatement is tests/iq_components_ref.py).  Normatively, for power_dev = rows * nfft floats, rows contiguous, in
 * the natural DFT order mdc_iq_spectrogram writes:
 *   centred    column c = (k + nfft/2) mod nfft of natural bin k: the order -0.5 .. 0.5 of a spectrum display.  The band is
 *              NOT circular: natural bins nfft-1 and 0 are neighbours (c = nfft/2 - 1 and nfft/2), natural bins nfft/2 - 1
 *              and nfft/2 are the two ends (c = nfft - 1 and 0).
 *   on         cell (r, c) is on iff power_dev[r*nfft + k] > thresh_dev[k], an f32 comparison: equality is off, a NaN on either
 *              side is off, a threshold of +Inf switches its bin off (a DC guard).
 *   link       two on-cells are linked iff |r1 - r2| <= reach_rows and |c1 - c2| <= reach_bins: reach (1, 1) is
 *              8-connectivity, a reach of g + 1 joins runs across a gap of g off cells, reach (0, 0) makes every on-cell a
 *              component of its own.  A component is a connected component of this graph.
 *   number     a component's root is its cell with the smallest r*nfft + c; components are numbered 0, 1, ... in ascending root.
 *   results    labels_dev[r*nfft + k] (the cell's natural position) is the number of the cell's component, -1 for an off cell;
 *              *count_dev is the number of components, whether or not they fit; comps_dev[i], i < min(count, capacity), is
 *              component i: row_first / row_stop and bin_first / bin_stop, its half-open bounding box in rows and CENTRED columns;
 *              cells, how many cells it has; peak, its largest value, and peak_row / peak_bin (centred), where that is.  "Largest"
 *              is mdc_iq_spectrum_quantiles' order of the bit patterns as unsigned integers -- the numeric order for everything
 *              a spectrogram produces --, and among equal patterns the cell with the smallest r*nfft + c wins.  Records at or
 *              beyond capacity are not written; the labels are complete regardless.
 * Everything is a function of the inputs alone: floats are only compared, never summed, and what is accumulated atomically
 * (integer minima, maxima and counts, the packed peak key) does not depend on the order of arrival -- the same bits on every run
 * and on every machine.
 * rows >= 1 and rows * nfft <= 2^31 - 1; nfft: a power of two in 64..4096; 0 <= reach_rows, reach_bins <= 4; capacity >= 0, and
 * capacity == 0 with comps_dev == NULL is legal (labels and count alone); no other buffer may be NULL.  power_dev, thresh_dev
 * (nfft floats) and labels_dev (rows * nfft int32) are 4-byte aligned, comps_dev (capacity records) and count_dev 8-byte
 * aligned; work_dev is 16-byte aligned and holds at least mdc_iq_spectrogram_components_workspace(rows, nfft) bytes (a 32-bit
 * counter per 1024 cells, rounded up to 16 bytes; negative MDC_EINVAL for a shape outside the limits; needs no device).  Its
 * contents are scratch: nothing is expected in it before the call and nothing is promised after.  Every argument error is
 * MDC_EINVAL before any device call.  The call only enqueues on hip_stream (no synchronisation, no allocation, no copy:
 * capturable in a hipGraph) and runs on the current device; no work-group waits for another. */
typedef struct mdc_iq_component {      /* 32 bytes */
    int32_t row_first, row_stop;       /* rows, half-open */
    int32_t bin_first, bin_stop;       /* centred columns, half-open */
    int32_t cells;
    float   peak;
    int32_t peak_row, peak_bin;        /* centred column */
} mdc_iq_component;

MDC_API int64_t mdc_iq_spectrogram_components_workspace(int64_t rows, int nfft);
MDC_API int mdc_iq_spectrogram_components(const float* power_dev, int64_t rows, int nfft, const float* thresh_dev, int reach_rows,
                                          int reach_bins, int32_t* labels_dev, mdc_iq_component* comps_dev, int64_t capacity,
                                          int64_t* count_dev, void* work_dev, void* hip_stream);

/* ---- spectrogram CFAR: a local order-statistic noise floor for every cell, and the ratio to it (additive in ABI 5) ----------
 * One threshold per bin for the whole capture follows neither a floor that moves in time (an AGC or gain step, a pulsed wideband
 * interferer) nor, where it is every bin's median over time, a continuous emitter on a coloured front-end.  The textbook answer
 * is a floor taken per CELL from the cells around it (2-D order-statistic CFAR): mdc_iq_spectrogram_cfar computes it for every
 * cell in one call, and the cell's ratio to it, which mdc_iq_spectrogram_components takes in the spectrogram's place (with a
 * threshold that is a plain factor).  The numpy restatement is tests/iq_cfar_ref.py.  Normatively, for power_dev = rows * nfft
 * floats, rows contiguous, in the natural DFT order mdc_iq_spectrogram writes:
 *   centred    column c = (k + nfft/2) mod nfft of natural bin k, mdc_iq_spectrogram_components' convention.  The band is NOT
 *              circular: natural bins nfft/2 - 1 and nfft/2 are the two ends (c = nfft - 1 and 0).
 *   training   the training set T of cell (r, c): all cells (r', c') of the spectrogram with |r' - r| <= train_rows and
 *              |c' - c| <= train_bins, minus those with |r' - r| <= guard_rows and |c' - c| <= guard_bins (the cell itself is
 *              always in the guard).  At the borders the window is cut off -- not wrapped, not padded --, so n = |T| varies; it
 *              is an integer function of (r, c, rows, nfft) alone.
 *   floor      the n 32-bit patterns of T are ordered ascending AS UNSIGNED INTEGERS, mdc_iq_spectrum_quantiles' order (the
 *              numeric order for everything a spectrogram produces; sign-bit and NaN patterns are ordered by the same rule, which
 *              is defined and memory-safe, if of no numeric use).  floor_dev[r*nfft + k] is the pattern at position
 *              ((n - 1) * rank_permille) / 1000 (0-based; the integer floor, taken in 64 bits): rank_permille 500 is the lower
 *              median, 0 the minimum, 1000 the maximum.  n == 0 gives +Inf.  Nothing is interpolated: the floor is an element of
 *              the spectrogram, the same bits on every run and on every machine.
 *   ratio      ratio_dev[r*nfft + k] = power_dev[r*nfft + k] / floor, ONE correctly rounded IEEE float32 division (no
 *              reciprocal, no fast-math).  0/0 and Inf/Inf are NaN, which mdc_iq_spectrogram_components reads as off; x/0, x > 0,
 *              is +Inf, which it reads as on; x / +Inf is 0: off.  Every NaN result is stored as the pattern 0x7FC00000 (IEEE
 *              leaves a NaN's sign and payload to the machine), so the ratio too is the same bits everywhere.
 * rows >= 1 and rows * nfft <= 2^31 - 1; nfft: a power of two in 64..4096; 0 <= guard_rows <= train_rows <= 16;
 * 0 <= guard_bins <= train_bins <= 128; (train_rows, train_bins) != (guard_rows, guard_bins); 0 <= rank_permille <= 1000.
 * floor_dev and ratio_dev hold rows * nfft floats each; either may be NULL (that output is not written), and both NULL is MDC_OK
 * with nothing launched (power_dev may then be NULL too).  Neither may overlap power_dev; all three are 4-byte aligned.  Every
 * argument error is MDC_EINVAL before any device call.  The call only enqueues on hip_stream (no synchronisation, no allocation,
 * no copy, no workspace: capturable in a hipGraph) and runs on the current device; no work-group waits for another. */
MDC_API int mdc_iq_spectrogram_cfar(const float* power_dev, int64_t rows, int nfft, int train_rows, int train_bins, int guard_rows,
                                    int guard_bins, int rank_permille, float* floor_dev, float* ratio_dev, void* hip_stream);

/* ---- channelizer: all M evenly spaced channels of a capture in one pass (additive in ABI 5) ---------------------------------
 * A band with a channel raster (PMR / LMR, GSM, FM broadcast, ISM sub-bands) wants every channel at once.  M calls of mdc_iq_ddc
 * read the capture M times and run M full-length filters; mdc_iq_channelizer is the polyphase filter bank that does it in one
 * pass: per output step the prototype filter once (T multiply-adds, shared by all channels) and one M-point transform (the
 * float64 numpy restatement is tests/iq_channelizer_ref.py).  Normatively, for the pairs_in = P input pairs x_n = (I_n, Q_n),
 * n counted from iq_dev, with M = channels, D = decimate, T = ntaps, s = tap_shift:
 *   widening   to 16-bit full scale, as in mdc_iq_ddc: MDC_IQ_CU8 (2*byte - 255)*128, MDC_IQ_CI8 s*256, MDC_IQ_CI16 s
 *              (|.| <= 32768; 0 dBFS stays 0 dBFS).
 *   taps       h_0 .. h_{T-1}: int16 at taps_dev (a DEVICE buffer, like the spectrogram's window: up to 32 KiB do not travel
 *              with a launch), applied as written (no reversal), in Q(15+s): DC gain 1 is a sum of 32768 * 2^s.  (A unit sum
 *              of 32768 spread over 8 M taps leaves the largest tap near 100 at M = 1024 and a stop band of 35 dB: the shift
 *              is what keeps the taps' precision.)
 *              Hard precondition, mdc_iq_resample's per-branch rule: for EVERY residue r in 0 .. M-1, sum_i |h_{r+iM}| <= 65535.
 *              The taps lie on the device and reading them back would be a synchronisation: the call does NOT validate them.
 *              The precondition is the caller's; with taps that break it the call is still memory-safe, only the values wrap.
 *   branch sums   for output j and residue r: v_j[r] = sum over t in 0 .. T-1 with (first_index + j D + t) mod M == r of
 *              h_t x_{jD+t}, re and im separately, int32; |v| <= 32768 * 65535 < 2^31: 32-bit accumulation is exact.  A residue
 *              without taps (possible when T < M) gives 0.
 *   transform  Y_j[k] = sum_r v_j[r] e^{-2 pi i k r / M}, k = 0 .. M-1, in float32 on v converted to f32, twiddle factors rounded
 *              from float64 (a table: no device sines).  This is
 *                  Y_j[k] = sum_t h_t x_{jD+t} e^{-2 pi i k (first_index + j D + t) / M}:
 *              channel k is the capture shifted by -k/M cycles per sample, the phase referenced to ABSOLUTE sample index 0
 *              (first_index is the absolute index of the pair at iq_dev), low-passed by h and decimated by D -- what mdc_iq_ddc
 *              does with phase_step = -k 2^32 / M and phase0 = first_index * phase_step, without its oscillator table's
 *              rounding.  Channel k is centred at k/M cycles per sample; k >= M/2 are the negative frequencies.
 *   output     out[k][j] = clamp(rint(Y_j[k] * 2^-(15+s)), -32768, 32767) (round half to even), re and im: int16 pairs,
 *              CHANNEL-MAJOR: out_dev holds M rows of n_out pairs, every row an ordinary MDC_IQ_CI16 capture for
 *              mdc_iq_windows / mdc_iq_windows_norm.  n_out = P >= T ? (P - T) / D + 1 : 0: a "valid" convolution.  The
 *              filter's group delay is not compensated.
 * With u = 2^-24 and eps = 8u (log2 M + 1) every output lies within 0.5 + eps S_j 2^-(15+s) of the unrounded, clamped
 * definition, S_j = sqrt(sum_k |Y_j[k]|^2) -- the spectrogram's bound, in amplitude form, plus the final rounding.
 * The same inputs give the same bits on every run; column j of a call does not depend on what else the call computes; a call on
 * the pairs from a on, a a multiple of D, with first_index + a returns the whole call's columns from j0 = a / D on, bit for
 * bit.
 * channels: a power of two in 8..1024; 1 <= decimate <= channels; 1 <= ntaps <= 16 * channels; 0 <= tap_shift <= 15;
 * first_index >= 0 (only its value mod M matters); n_out must equal mdc_iq_channelizer_out_count.  iq_dev is aligned to one
 * pair (2 / 2 / 4 bytes), taps_dev to 2 bytes, out_dev to 4 bytes.  Every argument error is MDC_EINVAL before any device call.
 * n_out == 0 is MDC_OK (nothing is launched; the buffers may be NULL); otherwise no buffer may be NULL.  The call only enqueues
 * on hip_stream (no synchronisation, no allocation, no copy: capturable in a hipGraph) and runs on the current device.
 * mdc_iq_channelizer_out_count returns n_out, or a negative MDC_EINVAL. */
MDC_API int64_t mdc_iq_channelizer_out_count(int64_t pairs_in, int channels, int ntaps, int decimate);
MDC_API int mdc_iq_channelizer(const void* iq_dev, int format, int64_t pairs_in, int64_t first_index, int channels, int decimate,
                               const int16_t* taps_dev, int ntaps, int tap_shift, int16_t* out_dev, int64_t n_out, void* hip_stream);

/* ---- frame synthesis: labelled I/Q frames of a balanced (modulation x SNR) grid, made on the device (additive in ABI 5) -------------
 * What cnn.py reads from RML2016.10a_dict.pkl (cnn.py:42-82) -- frames of 128 (I,Q) pairs, each with a modulation and an SNR --
 * generated instead of loaded: exact integers end to end, so the numpy restatement (tests/iq_synth_ref.py) is held bit for bit.
 * A frame is 128 MDC_IQ_CI16 pairs.  Its content is a function of (recipe, seed, absolute frame index f) and of nothing else:
 * not of n_frames, not of the frame's place in the call, not of the launch.  f = first_frame + i (mod 2^64) for frame i of a call.
 *   labels     the recipe has C classes and S SNR entries: cell = f mod (C S), class = cell mod C, snr_index = cell / C.  Any C S
 *              consecutive frames are one exactly balanced grid.  No randomness goes into labels.
 *   generator  counter-based on fmix32 (mdc_trainer_set_dropout, below, states it).  With seed and f split into 32-bit words,
 *                  k_seed = fmix32(fmix32(seed_lo + 0x9E3779B9) ^ seed_hi)
 *                  key_f  = fmix32(fmix32(k_seed ^ (f_lo * 0x85EBCA6B)) ^ (f_hi * 0x85EBCA6B + 1))
 *              (all mod 2^32), and draw j of the frame is d(j) = fmix32(key_f + j * 0xC2B2AE35).  The counters:
 *                  j = 0              timing offset   tau   = (d * sps) >> 32                     (64-bit product; 0 <= tau < sps)
 *                  j = 1              carrier phase   phi0  = d
 *                  j = 2              carrier step    step  = ((d * (2 max_step + 1)) >> 32) - max_step   (then mod 2^32)
 *                  j = 3              PHASE start     theta0 = d
 *                  j = 16 + 4 k + e   source symbol k (e = 0 .. 3; an alphabet uses e = 0 only), k = 0 .. 143
 *                  j = 1024 + 8 n + 4 c + e   noise of output sample n, component c (0 = I, 1 = Q), e = 0 .. 3
 *              g(d0 .. d3) = sum over the four draws of (d & 0xFFFF) + (d >> 16), minus 262140: eight uniform 16-bit integers,
 *              mean 0, variance 8 (2^32 - 1) / 12 exactly, |g| <= 262140.
 *   source     per class, symbol k is a complex integer a_k: MDC_SYNTH_ALPHABET: point number (d(16 + 4k) * M) >> 32 of the class's
 *              M points (int16 pairs; M a power of two in 1..64); MDC_SYNTH_GAUSS: a_k = (g(d(16 + 4k) .. d(16 + 4k + 3)), 0).
 *   pulse      sps * span complex int16 Q15 taps h_0 .. (1 <= sps <= 16, 1 <= span <= 16, sps * span <= 128), given in natural order;
 *              the plan stores them branch-major (branch b = h_b, h_{b+sps}, ...), as the resampler stores its taps.  Output sample n
 *              of the frame sits at p = n + tau of the symbol stream: with m = p / sps and b = p mod sps,
 *                  y_n = (sum over i in 0 .. span-1 of a_{m + span - 1 - i} * h_{b + i sps}  +  2^14 (1 + j)) >> 15
 *              -- complex products, re and im accumulated in int64, ONE rounding shift (arithmetic, i.e. floor) per component.  The
 *              span - 1 symbols before the frame that the pulse still reaches are drawn like the others: no ramp-up inside a frame.
 *              Hard precondition, checked by the plan: for every branch b, B_b = amax * sum_i (|re h_{b+i sps}| + |im h_{b+i sps}|)
 *              with amax = the largest |component| of the alphabet (262140 for MDC_SYNTH_GAUSS) satisfies
 *              ((B_b + 2^14) >> 15) + max(|add_re|, |add_im|) <= 32767: y_n + add fits int16 (and 32-bit accumulation is exact too).
 *   mode       MDC_SYNTH_LINEAR: z_n = y_n + add (add: the class's complex int16 constant -- AM's carrier).
 *              MDC_SYNTH_PHASE:  inc_n = (re y_n * phase_factor) mod 2^32; theta_n = theta0 + inc_0 + ... + inc_n (mod 2^32, the sum
 *              INCLUDES inc_n); (c, s) = the oscillator table's entry theta_n >> 20 (mdc_iq_ddc_nco_table, mdc_iq_ddc's rule);
 *              z_n = ((c * amplitude + 2^14) >> 15, (s * amplitude + 2^14) >> 15) + add; |amplitude| + max|add| <= 32767 (checked).
 *   channel    phi_n = phi0 + n * step (mod 2^32), (c, s) = table entry phi_n >> 20, and the mixer of mdc_iq_ddc, word for word:
 *                  m_n = ((re z c - im z s + 32768) >> 16, (re z s + im z c + 32768) >> 16)            (z e^{j phi} / 2)
 *              then, per component, in int64, with w = g(the component's four noise draws):
 *                  out = clamp((m * gain_sig[class * S + snr_index] + w * gain_noise[snr_index] + 2^(q-1)) >> q, -32768, 32767)
 *              Every component the clamp changes is counted into *saturated_dev (+=, one uint64; the caller zeroes it).
 * Stated limit: the noise is an Irwin-Hall sum of eight uniforms, not a Gaussian: excess kurtosis -0.15, no sample beyond
 * 262140 / sqrt(8 (2^32 - 1) / 12) = 4.9 sigma.  mdc_iq_synth_frames has no multipath fading (mdc_iq_synth_frames_faded, below, has),
 * and neither entry has sample-rate drift or a carrier random walk: at the magnitudes the RML2016.10a generator uses, the drift moves
 * a 128-sample frame by hundredths of a sample, and the walk stays inside the offset that max_step already draws per frame.
 *
 * mdc_iq_synth_plan (host code, no GPU) validates a recipe and writes the plan blob (position-independent: offsets from its first
 * byte; copy it anywhere, hand mdc_iq_synth_frames the same bytes in host and in device memory).  classes_host: C records, 1 <= C
 * <= 64; points_host: npoints int16 PAIRS, a class's alphabet being pairs first_point .. first_point + points - 1; taps_host: ntaps
 * int16 PAIRS (re, im), a class's pulse being pairs first_tap .. first_tap + sps * span - 1; gain_sig_host: ngain_sig int32, which
 * must equal C * nsnrs (class-major); gain_noise_host: nsnrs int32, 1 <= nsnrs <= 64; max_step <= 2^30; 1 <= q <= 40; reserved
 * fields 0.  plan_bytes must equal mdc_iq_synth_plan_bytes(C, nsnrs, classes_host), which depends on the records' shapes only
 * (a negative MDC_EINVAL for shapes the plan would refuse).  Every refusal is MDC_EINVAL with an error text that names the class.
 * mdc_iq_synth_frames: iq_out_dev takes n_frames * 128 pairs (4-byte aligned); labels_dev / snr_index_dev (n_frames int32 each) and
 * saturated_dev (8-byte aligned) may be NULL; 0 <= n_frames <= 2^30; n_frames == 0 is MDC_OK without a launch.  plan_dev is 8-byte
 * aligned.  The call only enqueues on hip_stream (no synchronisation, no allocation, no copy: capturable in a hipGraph) and runs
 * on the current device.  The same arguments give the same bits on every run. */
#define MDC_SYNTH_ALPHABET 0
#define MDC_SYNTH_GAUSS 1
#define MDC_SYNTH_LINEAR 0
#define MDC_SYNTH_PHASE 1
typedef struct mdc_iq_synth_class {
    int32_t source;            /* MDC_SYNTH_ALPHABET / MDC_SYNTH_GAUSS */
    int32_t points;            /* M: alphabet size (a power of two in 1..64); 0 for MDC_SYNTH_GAUSS */
    int32_t first_point;       /* the alphabet's first pair in points_host */
    int32_t sps, span;         /* samples per symbol, pulse length in symbols */
    int32_t first_tap;         /* the pulse's first pair in taps_host */
    int32_t mode;              /* MDC_SYNTH_LINEAR / MDC_SYNTH_PHASE */
    int32_t phase_factor;      /* MDC_SYNTH_PHASE: phase increment per unit of re y */
    int16_t amplitude;         /* MDC_SYNTH_PHASE: the carrier's amplitude */
    int16_t add_re, add_im;    /* constant added after filtering / to the carrier */
    int16_t reserved;          /* 0 */
} mdc_iq_synth_class;          /* 40 bytes */
MDC_API int64_t mdc_iq_synth_plan_bytes(int32_t nclasses, int32_t nsnrs, const mdc_iq_synth_class* classes_host);
MDC_API int mdc_iq_synth_plan(const mdc_iq_synth_class* classes_host, int32_t nclasses, const int16_t* points_host, int64_t npoints,
                              const int16_t* taps_host, int64_t ntaps, const int32_t* gain_sig_host, int64_t ngain_sig,
                              const int32_t* gain_noise_host, int32_t nsnrs, uint32_t max_step, int32_t q, void* plan_host,
                              int64_t plan_bytes);
MDC_API int mdc_iq_synth_frames(const void* plan_host, const void* plan_dev, int64_t plan_bytes, uint64_t seed, uint64_t first_frame,
                                int64_t n_frames, int16_t* iq_out_dev, int32_t* labels_dev, int32_t* snr_index_dev,
                                uint64_t* saturated_dev, void* hip_stream);

/* ---- frame synthesis through a frequency-selective Rician channel (additive in ABI 5) ------------------------------------------------
 * mdc_iq_synth_frames_faded: the frames of mdc_iq_synth_frames, sent through P delayed paths with random complex gains before the
 * gains and the noise.  The plan, its blob, the labels, the generator, the noise counters and the saturation count are those of
 * mdc_iq_synth_frames, word for word; a frame stays a function of (recipe, fading record, seed, f) alone, in exact integers
 * (the numpy restatement is tests/iq_synth_fading_ref.py).  fading_host is read and validated during the call and travels with the
 * launch: no device copy.  With T = taps, H = T - 1:
 *   head       the unfaded chain runs for n' = 0 .. 127 + H with its formulas unchanged and gives m_{n'}: source, pulse at p = n' + tau,
 *              mode (PHASE's running sum runs H samples longer), mixer at phi0 + n' step.  A frame draws
 *              (127 + H + sps - 1) / sps + span symbols, at most 159; their counters stay j = 16 + 4 k + e <= 651.
 *   gains      per frame and path p, at the counters j = 768 + 16 p + e (free in mdc_iq_synth_frames: symbols end below 768, noise
 *              starts at 1024): G_p = (g(d(e = 0 .. 3)), g(d(e = 4 .. 7))), the noise's own sum, and per component
 *                  g_p = los_p + ((G_p * scatter_p + 2^17) >> 18)                      (int64 product; Q13: 8192 is a gain of one)
 *              |G| <= 262140 < 2^18 gives |(G scatter + 2^17) >> 18| <= scatter, so with the precondition
 *              max(|los_re|, |los_im|) + scatter <= 32767 every component of g_p fits int16.
 *   Doppler    only if max_doppler_step > 0: psi_p = d(e = 8); nu_p = ((d(e = 9) * (2 max_doppler_step + 1)) >> 32) - max_doppler_step
 *              (mod 2^32, as `step` is drawn); (c, s) = the oscillator table's entry (psi_p + n nu_p) >> 20 for output sample n, and
 *                  r_p(n) = ((re g c - im g s + 2^14) >> 15, (re g s + im g c + 2^14) >> 15)
 *              Otherwise r_p(n) = g_p and no table is read.  |re g c - im g s| <= |g| |(c, s)| <= 32767 sqrt(2) * 32768 < 2^31 (int32
 *              is exact), and every component of r is below 46341 in absolute value (32767 sqrt(2) + 1/2 < 46341; the table's entries
 *              have c^2 + s^2 <= 32768^2).
 *   delay      per path T real int16 Q14 taps d_p[0 .. T-1]:  u_p(n) = (sum over k of d_p[k] * m_{n + H - k}  +  2^13) >> 14 per
 *              component.  Precondition: sum_k |d_p[k]| <= 32767; with |m| <= 32768 per component the sum stays below 2^30 (int32 is
 *              exact) and |u| <= 65537.  d_p[k] = 16384 at one k and 0 elsewhere is a delay of k samples, exactly.
 *   sum        y_n = (sum over p of r_p(n) * u_p(n)  +  2^12 (1 + j)) >> 13 -- complex products, re and im accumulated in int64, ONE
 *              rounding shift per component.  |y| <= (4 * 2 * 46341 * 65537 + 2^12) >> 13 < 2^22.
 *   output     y_n takes m_n's place:  out = clamp((y * gain_sig + w * gain_noise + 2^(q-1)) >> q, -32768, 32767), the same noise
 *              counters and the same count.  |y gain_sig| < 2^53 and |w gain_noise| < 2^49: the sum stays below 2^62.
 * (The path gains are Q13 and the sum shifts by 13, where a first draft had Q14 and 14: a component of g is at most 32767 and the
 * Irwin-Hall sum reaches 4.9 sigma, so Q14 would cap a path's scattered power at 2 (0.408)^2 = 0.33 of the whole channel's -- below
 * the second path of the RML2016.10a profile, 0.37.  Q13 takes any path of a channel of unit power.)
 * Stated limit: the Doppler is ONE rotating phasor per path (a frequency offset drawn per frame and path), not a sum of sinusoids
 * with a Jakes spectrum; the scattered part of a gain is the Irwin-Hall sum above, not a Gaussian, and constant over the frame; the
 * SNR a frame is labelled with is the AVERAGE over the fading -- a frame's own SNR varies with its gains, which is the point; no
 * sample-rate drift and no carrier walk (see above).
 * mdc_iq_synth_fading: 1 <= paths <= 4; 1 <= taps <= 16; max_doppler_step <= 2^30; per path p < paths the two preconditions above and
 * scatter >= 0; delay_taps[k] = 0 for k >= taps; every field of a path p >= paths and every reserved field 0.  fading_host must not
 * be NULL.  The record is checked first, also when n_frames == 0, so a record can be validated without a device;
 * every refusal is MDC_EINVAL before any device call, with an error text that names the path.  All else as mdc_iq_synth_frames. */
typedef struct mdc_iq_synth_path {
    int16_t delay_taps[16];    /* d_p[k], real, Q14 (16384 = 1) */
    int16_t los_re, los_im;    /* the constant (line-of-sight) part of the gain, Q13 (8192 = 1) */
    int32_t scatter;           /* >= 0: scale of the drawn part, per component 53510 / 2^18 * scatter rms (Q13) */
    int32_t reserved[2];       /* 0 */
} mdc_iq_synth_path;           /* 48 bytes */
typedef struct mdc_iq_synth_fading {
    int32_t paths, taps;       /* P, T */
    uint32_t max_doppler_step; /* per path, nu is drawn in -max .. max (2^32 = one cycle per sample); 0: no Doppler */
    int32_t reserved;          /* 0 */
    mdc_iq_synth_path path[4];
} mdc_iq_synth_fading;         /* 208 bytes */
MDC_API int mdc_iq_synth_frames_faded(const void* plan_host, const void* plan_dev, int64_t plan_bytes, uint64_t seed, uint64_t first_frame,
                                      int64_t n_frames, int16_t* iq_out_dev, int32_t* labels_dev, int32_t* snr_index_dev,
                                      uint64_t* saturated_dev, const mdc_iq_synth_fading* fading_host, void* hip_stream);

/* ---- capture synthesis: a scene of emitters rendered into one wideband MDC_IQ_CI16 capture (additive in ABI 5) -----------------------
 * The inverse of mdc_iq_extract: E emitters, each a class of a plan of mdc_iq_synth_plan with a rate, a carrier (or a hop set), a
 * level and a burst schedule, summed with noise into ONE capture -- exact integers end to end, so the numpy restatement
 * (tests/iq_synth_capture_ref.py) is held bit for bit.  Capture sample n is a function of (plan, scene, seed, n) alone.  Of the plan
 * only the class records, alphabets and tap images are used; its gain tables, q and max_step are not.
 *   draws      those of "frame synthesis": key = key_f with k_seed of the seed, d(j) = fmix32(key + j * 0xC2B2AE35), with f composed
 *              per purpose (e: the emitter's index; fields do not overlap: the low part stays below 2^52):
 *                  f = (e+1) 2^56 + 0 2^52 + (k >> 7)   symbol k >= 0 of emitter e; counters 16 + 4 (k & 127) + e', e' = 0 .. 3, used
 *                                                       as the frames use 16 + 4 k + e' (an alphabet uses e' = 0 only)
 *                  f = (e+1) 2^56 + 1 2^52              the emitter's constants: j = 0: tau = (d * sps) >> 32; j = 3: theta0 = d
 *                  f = (e+1) 2^56 + 2 2^52 + w          dwell w: j = 0: hop index = (d * hops) >> 32
 *                  f =          3 2^52 + (n >> 7)       noise of capture sample n: counters 1024 + 8 (n & 127) + 4 c + e', and g()
 *   baseband   per emitter a stream z_i, i >= 0, at the class's sps: the source, pulse and mode lines of "frame synthesis", word for
 *              word, at p = i + tau, with symbol indices k = p / sps + span - 1 - t unbounded above (and >= 0: no ramp-up).
 *              MDC_SYNTH_PHASE: theta_i = theta0 + inc_0 + ... + inc_i (mod 2^32) over ALL i from 0, gated-off stretches included:
 *              a continuous-phase emitter's phase is continuous across the whole capture.  |z| <= 32767 per component (the plan's
 *              preconditions).
 *   gate       start, on, period >= 0, in baseband samples.  The emitter is on at i iff i >= start and either period == 0 and
 *              (on == 0 or i - start < on), or period > 0 and (i - start) mod period < on.  zg_i = z_i when on, else 0.  The dwell
 *              of i is w(i) = (i - start) / period when period > 0 and i >= start, else 0.  The gate acts BEFORE the interpolation
 *              filter, which therefore shapes the burst edges.
 *   rate       L = interpolate, D = decimate (1 <= D <= L <= 32: an emitter is never decimated), T = ntaps real int16 Q15 taps h of
 *              the scene's tap array, given in natural order.  For capture sample n: P = n D + T - 1, m = P / L, r = P mod L,
 *                  acc_n = sum over i >= 0 with r + i L < T of h[r + i L] * zg_{m - i}            (re and im separately)
 *              Every index m - i is >= 0 (i <= (T - 1 - r) / L gives m - i >= (P - T + 1) / L >= 0): no start-up ramp, no history.
 *              Preconditions: ceil(T / L) <= 64, and for every branch r the sum over i of |h[r + i L]| <= 65535 (mdc_iq_resample's
 *              bound): |acc| <= 32767 * 65535 < 2^31, 32-bit accumulation is exact.  u_n = clamp16((acc_n + 2^14) >> 15); clamped
 *              components count into *saturated_dev.  Taps of frontend.design_resampler(L, D) (every branch sums to 32768) pass.
 *   carrier    hops carriers phase_step[0 .. hops-1]; the one in use at n is that of the dwell of the LATEST baseband sample the
 *              filter reads: h_n = hop index of w(m) (0 when hops == 1).  phi_n = phase0 + n * phase_step[h_n] (mod 2^32), referenced
 *              to capture sample 0 whatever the schedule; (c, s) = the oscillator table's entry phi_n >> 20, and the mixer of
 *              mdc_iq_ddc, word for word:  m_{e,n} = ((re u c - im u s + 32768) >> 16, (re u s + im u c + 32768) >> 16), |.| <= 32768.
 *              hops > 1 requires period > 0 (a dwell is one period).
 *   sum        per component, in int64, with w_n = g(the component's four noise draws):
 *                  out_n = clamp(((sum over e of m_{e,n} * gain_e + w_n * gain_noise + 2^(q-1)) >> q) + dc, -32768, 32767)
 *              Bound: 32 emitters * 32768 * 2^31 = 2^51, |w gain_noise| < 2^18 * 2^31 = 2^49, 2^(q-1) <= 2^39: |sum| < 2^52 < 2^62.
 *              After the shift |.| < 2^51, so adding dc cannot wrap either.  Components the clamp changes are counted as well.
 * Properties: the capture always starts at sample 0; a capture of n1 pairs is the first n1 pairs of a capture of n2 > n1 pairs, bit
 * for bit (the count of clamped components is that of the pairs written); the same arguments give the same bits on every run; an
 * emitter's m_{e,n} does not depend on which other emitters the scene holds, only on its own index e; E == 0 gives noise plus dc.
 * Resuming at a sample other than 0 is out of scope: MDC_SYNTH_PHASE would need a carried phase.
 * Truth: baseband sample i of an emitter is centred on capture sample (2 i L - (T - 1)) / (2 D) (the filter's centre, (T - 1) / 2
 * interpolated samples); frontend.scene_truth rounds it half up, floor((2 i L - (T - 1) + D) / (2 D)), and clamps at 0.
 *
 * mdc_iq_synth_scene (host code, no GPU) validates a scene against its plan and writes the position-independent scene blob; hand
 * mdc_iq_synth_capture the same bytes in host and in device memory, with the plan the scene was built for.  0 <= nemitters <= 32;
 * taps_host: ntaps int16, 0 <= ntaps <= 32768; gain_noise >= 0; 1 <= q <= 40; per emitter: 0 <= cls < the plan's classes, 1 <=
 * decimate <= interpolate <= 32, 1 <= ntaps <= 1024 inside taps_host, the two tap preconditions above, 1 <= hops <= 8, start, on,
 * period in 0 .. 2^52, reserved 0.  scene_bytes must equal mdc_iq_synth_scene_bytes(nemitters, ntaps).  Every refusal is MDC_EINVAL
 * with an error text that names the emitter.
 * mdc_iq_synth_scene_hops (host code, no GPU): hop_index_out[i] = the hop index of dwell first_dwell + i of `emitter`, i < n.
 * mdc_iq_synth_capture: out_dev takes n_pairs pairs (4-byte aligned); saturated_dev (8-byte aligned, +=, the caller zeroes it) may be
 * NULL; scene_dev and plan_dev are 8-byte aligned; workspace_dev (4-byte aligned) holds at least
 * mdc_iq_synth_capture_workspace_bytes(scene, n_pairs) bytes (0 for a scene without an MDC_SYNTH_PHASE emitter; NULL is then
 * accepted) and needs no initialisation; 0 <= n_pairs <= 2^34; n_pairs == 0 is MDC_OK without a launch.  The call only enqueues on
 * hip_stream (no synchronisation, no allocation, no copy: capturable in a hipGraph) and runs on the current device. */
typedef struct mdc_iq_synth_emitter {
    int32_t cls;               /* index into the plan's classes */
    int32_t interpolate;       /* L, 1..32 */
    int32_t decimate;          /* D, 1..L */
    int32_t first_tap, ntaps;  /* the interpolation filter: taps first_tap .. first_tap + ntaps - 1 of the scene's tap array */
    int32_t gain;              /* gain_e */
    uint32_t phase0;           /* carrier phase at capture sample 0 */
    int32_t hops;              /* carriers in use, 1..8 */
    uint32_t phase_step[8];    /* the carriers (2^32 = one cycle per capture sample) */
    int64_t start, on, period; /* burst schedule, in baseband samples */
    int32_t reserved[2];       /* 0 */
} mdc_iq_synth_emitter;        /* 96 bytes */
MDC_API int64_t mdc_iq_synth_scene_bytes(int32_t nemitters, int64_t ntaps);
MDC_API int mdc_iq_synth_scene(const void* plan_host, int64_t plan_bytes, const mdc_iq_synth_emitter* emitters_host, int32_t nemitters,
                               const int16_t* taps_host, int64_t ntaps, int32_t gain_noise, int32_t q, int16_t dc_re, int16_t dc_im,
                               void* scene_host, int64_t scene_bytes);
MDC_API int mdc_iq_synth_scene_hops(const void* scene_host, int64_t scene_bytes, uint64_t seed, int32_t emitter, int64_t first_dwell,
                                    int64_t n, int32_t* hop_index_out);
MDC_API int64_t mdc_iq_synth_capture_workspace_bytes(const void* scene_host, int64_t scene_bytes, int64_t n_pairs);
MDC_API int mdc_iq_synth_capture(const void* scene_host, const void* scene_dev, int64_t scene_bytes, const void* plan_host,
                                 const void* plan_dev, int64_t plan_bytes, uint64_t seed, int64_t n_pairs, int16_t* out_dev,
                                 uint64_t* saturated_dev, void* workspace_dev, int64_t workspace_bytes, void* hip_stream);

/* test_Y_hat = model.predict(X_test, batch_size=batch_size)  (cnn.py:198, 237) when X_test lies in HOST memory -- a
 * numpy array, or whatever buffer a cgo / JNI / N-API caller holds: the library's own driver in front of mdc_forward.
 * Frames are copied into a pinned ring by a few host threads, DMA'd, computed and the results DMA'd back in three
 * overlapping slots of chunk_frames frames (0 = 65,536) on the library's own streams, so the call runs at
 * max(PCIe, kernel) rather than their sum; x_host that is already pinned (hipHostMalloc / hipHostRegister) is DMA'd
 * from where it lies.  SYNCHRONOUS, like Keras' predict: returns when probs_host (n,C) f32 and labels_host (n) int32
 * (each may be NULL) are complete.  Results are bit-identical to mdc_forward on the same frames, whatever the chunk.
 * Staging buffers, streams and the workspace belong to the model (created on first use, freed by mdc_destroy); calls
 * on one model are serialised.  Added in ABI 2 (additive). */
MDC_API int mdc_predict_host(mdc_model* m, const float* x_host, int64_t n, float* probs_host, int32_t* labels_host,
                     int64_t chunk_frames);

/* The same for raw uint8 I/Q in host memory (an SDR capture buffer, README.md:5): n windows, `hop` pairs apart, from
 * iq_host (2*hop*(n-1) + 256 bytes) through mdc_forward_iq_u8 -- 2*hop bytes per window over PCIe instead of 1,024. */
MDC_API int mdc_predict_host_iq_u8(mdc_model* m, const uint8_t* iq_host, int64_t n, int64_t hop, float scale,
                           float* probs_host, int32_t* labels_host, int64_t chunk_frames);

/* The same through mdc_iq_u8_windows_norm + mdc_forward: each slot's bytes are normalised into a frame buffer of the
 * model's host context (freed by mdc_destroy; a default chunk keeps it within 64 MiB per slot) and forwarded from there, so
 * every kind is served, MDC_KIND_CNNPY included.  level / flags as mdc_iq_u8_windows_norm; stats_host (n) receives the
 * windows' statistics, or is NULL.  Results are bit-identical to the two device calls on the same bytes, whatever the
 * chunk. */
MDC_API int mdc_predict_host_iq_u8_norm(mdc_model* m, const uint8_t* iq_host, int64_t n, int64_t hop, float level, int flags,
                           float* probs_host, int32_t* labels_host, mdc_iq_window_stats* stats_host,
                           int64_t chunk_frames);

/* The two drivers above for a capture in any MDC_IQ_* format (iq_host: (hop*(n-1) + 128) pairs of 2 / 2 / 4 bytes; a
 * misaligned pointer is copied as it is: only the device side wants whole pairs).  Both go through frames -- mdc_iq_windows /
 * mdc_iq_windows_norm into the slot's frame buffer, then mdc_forward -- so every kind is served, MDC_KIND_CNNPY included,
 * and the results are bit-identical to those two device calls on the same samples, whatever the chunk.  stats64_host (n)
 * receives the windows' 64-bit statistics, or is NULL.  (MDC_IQ_CU8 through mdc_predict_host_iq is
 * mdc_predict_host_iq_u8 where that serves the model's kind.) */
MDC_API int mdc_predict_host_iq(mdc_model* m, const void* iq_host, int format, int64_t n, int64_t hop, float scale,
                           float* probs_host, int32_t* labels_host, int64_t chunk_frames);
MDC_API int mdc_predict_host_iq_norm(mdc_model* m, const void* iq_host, int format, int64_t n, int64_t hop, float level, int flags,
                           float* probs_host, int32_t* labels_host, mdc_iq_window_stats64* stats64_host,
                           int64_t chunk_frames);

/* Measurement support (bench.py roofline leg): when on, mdc_forward brackets each kernel
 * launch with HIP events on the launch stream; mdc_profile_read synchronises on them and
 * returns the summed device time and launch count of kernel slot `slot` since the last
 * mdc_profile_reset.  Off by default; never on in the timed region of the headline number.
 * Forwards may run concurrently with profiling on (the event lists are mutex-guarded); mdc_set_profiling /
 * mdc_profile_reset themselves must not race with forwards of the same model. */
MDC_API int mdc_set_profiling(mdc_model* m, int on);
MDC_API int mdc_profile_slots(const mdc_model* m);
MDC_API const char* mdc_profile_name(const mdc_model* m, int slot);
MDC_API int mdc_profile_read(mdc_model* m, int slot, double* total_ms, int64_t* launches);
MDC_API int mdc_profile_reset(mdc_model* m);

/* ---- training -----------------------------------------------------------------------
 * The reference trains two nets: CNN.ipynb cell 6's (MDC_KIND_DEPLOYED; the five bundled .h5 files are its results) and
 * cnn.py:104-112's (MDC_KIND_CNNPY).  Neither contains a Dropout layer, so the training forward is the inference
 * forward.  MDC_KIND_VTCNN2 is refused (MDC_ENOTSUP): its training exists only in the vendored DeepSig notebook.  f32.
 *
 *     model.compile(loss='categorical_crossentropy', optimizer='adam')     cnn.py:113     mdc_trainer_create (+ _set_adam)
 *     (the freshly initialised / loaded weights)                            cnn.py:108-111 mdc_trainer_set_tensor(MDC_TRAIN_WEIGHTS)
 *     model.fit(...): one mini-batch of one epoch                           cnn.py:135     mdc_train_batch
 *     ... validation_data=(X_test, Y_test): val_loss after each epoch       cnn.py:140     mdc_trainer_evaluate + mdc_trainer_read
 *     ModelCheckpoint(filepath, save_best_only=True) / load_weights         cnn.py:143-147 mdc_trainer_get_tensor (weights, Adam m / v,
 *                                                                                          iterations: all a Keras full-model .h5 holds)
 * The loss is Keras 2.4's categorical_crossentropy on the softmax OUTPUT (the model ends in Activation('softmax') +
 * Reshape, so the loss sees probabilities): q = p / sum(p), clipped to [1e-7, 1 - 1e-7], L = -sum_c y_c log q_c, mean over
 * the batch; the clip passes no gradient outside its interval, a ReLU none where its input is <= 0.  The optimizer is
 * TensorFlow 2.4's Adam: alpha = lr sqrt(1 - beta2^t) / (1 - beta1^t), m += (g - m)(1 - beta1), v += (g g - v)(1 - beta2),
 * w -= m alpha / (sqrt(v) + eps) with t = iterations + 1 (eps is NOT scaled by the bias correction).
 * Everything below runs on the trainer's device; x_dev (frames (., 2, 128) f32, 16-byte aligned) and y_dev (target rows
 * (., classes) f32: the one-hot rows of cnn.py:74-82, or any distribution) are the caller's buffers holding the WHOLE set;
 * a mini-batch is the frames order_dev[first .. first + count) of it (order_dev: int32 indices on the device, the
 * epoch's shuffle -- frames are never moved; NULL = the identity).  n_frames is how many frames the two buffers hold: a
 * position whose index lies outside [0, n_frames) is SKIPPED on the device -- it adds nothing to the loss or the gradient
 * (the batch mean still divides by count) -- and is counted; the next mdc_trainer_read then returns MDC_EINVAL with the count:
 * a bad shuffle is an error at the epoch's read, never a GPU fault.  mdc_train_batch and mdc_trainer_evaluate only enqueue
 * on hip_stream (two launches, no synchronisation, no allocation: capturable in a hipGraph; Adam's step count lives on the
 * device).  A step is reproducible bit for bit (fixed-order reductions, no float atomics).  One stream at a time per trainer. */
typedef struct mdc_trainer mdc_trainer;   /* opaque: f32 master weights in the Keras layouts, Adam state, scratch */

MDC_API int mdc_trainer_create(const mdc_topology* topo, int device, mdc_trainer** out);
MDC_API int mdc_trainer_num_layers(const mdc_trainer* t);
MDC_API int mdc_trainer_layer_sizes(const mdc_trainer* t, int layer, size_t* kernel_elems, size_t* bias_elems);

/* keras.optimizers.Adam(lr, beta_1, beta_2, epsilon); the defaults (1e-3, 0.9, 0.999, 1e-7 -- what 'adam' at cnn.py:113
 * means and what every bundled .h5's training_config records) hold until this is called. */
MDC_API int mdc_trainer_set_adam(mdc_trainer* t, float lr, float beta1, float beta2, float eps);

/* OPTIONAL Dropout(rate), off by default (rate 0 = the nets as the reference defines them: cnn.py:104-112 and CNN.ipynb cell 6
 * contain no Dropout layer; their `dr = 0.5` / `0.6` is left over from the DeepSig definition, which has `model.add(Dropout(dr))`
 * behind every conv and behind dense1 -- RML2016.10a_VTCNN2_example.ipynb:229-243).  With rate > 0 the training batches
 * (mdc_train_batch, either value of `apply`) multiply the conv + ReLU output -- and, for MDC_KIND_CNNPY, the Dense(D, relu)
 * output -- by mask / (1 - rate), Keras' Dropout; mdc_trainer_evaluate and every mdc_forward* never do (inference).  TensorFlow's
 * generator cannot be replayed, so the mask comes from a stated counter-based one (uint32 arithmetic):
 *     fmix32(h):  h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16
 *     k_step  = fmix32(seed + 0x9E3779B9 * (iterations + 1))          iterations: Adam's step count (on the device)
 *     k_frame = fmix32(k_step ^ (frame * 0x85EBCA6B + site))          frame: the frame's index in x_dev; site 0 conv, 1 dense
 *     keep element e (its index in the layer's Flatten order) iff fmix32(k_frame + e * 0xC2B2AE35) >= floor(rate * 2^32)
 * -- a new mask at every step (also under hipGraph replay), the same mask for a frame whatever batch it arrives in. */
MDC_API int mdc_trainer_set_dropout(mdc_trainer* t, float rate, uint32_t seed);

/* Per-layer tensors in the layouts of mdc_set_weights.  MDC_TRAIN_WEIGHTS must be set for every layer before the first
 * batch; Adam's moments start at zero and `iterations` at 0 (set them to resume from a full-model .h5, whose
 * /optimizer_weights group holds exactly these).  MDC_TRAIN_GRADIENT (get only): d(mean loss)/d(weights) of the last
 * mdc_train_batch.  Both calls synchronise hip_stream (the host buffers are complete / reusable on return). */
enum { MDC_TRAIN_WEIGHTS = 0, MDC_TRAIN_ADAM_M = 1, MDC_TRAIN_ADAM_V = 2, MDC_TRAIN_GRADIENT = 3 };
MDC_API int mdc_trainer_set_tensor(mdc_trainer* t, int which, int layer, const float* kernel_host, size_t kernel_elems,
                           const float* bias_host, size_t bias_elems, void* hip_stream);
MDC_API int mdc_trainer_get_tensor(mdc_trainer* t, int which, int layer, float* kernel_host, size_t kernel_elems,
                           float* bias_host, size_t bias_elems, void* hip_stream);
MDC_API int mdc_trainer_set_iterations(mdc_trainer* t, int64_t iterations, void* hip_stream);

/* model.train_on_batch / one step of model.fit (cnn.py:135): forward, loss, backward over the `count` frames and, if
 * `apply` != 0, one Adam update (apply = 0: the gradient is computed and kept for MDC_TRAIN_GRADIENT, nothing changes).
 * The batch's summed loss and frame count are added to the trainer's running training statistics. */
MDC_API int mdc_train_batch(mdc_trainer* t, const float* x_dev, const float* y_dev, int64_t n_frames, const int32_t* order_dev,
                    int64_t first, int64_t count, int apply, void* hip_stream);

/* The val_loss half of model.fit's epoch end / model.evaluate with the weights as they are now (cnn.py:140, 153): adds the
 * summed per-sample loss and the frame count to the trainer's evaluation statistics. */
MDC_API int mdc_trainer_evaluate(mdc_trainer* t, const float* x_dev, const float* y_dev, int64_t n_frames, const int32_t* order_dev,
                         int64_t first, int64_t count, void* hip_stream);

/* Synchronise hip_stream and read the statistics (each pointer may be NULL): sums of per-sample losses and frame counts
 * since the last reset, for training batches and for evaluation (mean = sum / frames: fit's `loss` and `val_loss`), and
 * Adam's step count.  reset != 0 zeroes the four statistics (not `iterations`). */
MDC_API int mdc_trainer_read(mdc_trainer* t, int reset, double* train_loss_sum, int64_t* train_frames, double* eval_loss_sum,
                     int64_t* eval_frames, int64_t* iterations, void* hip_stream);

MDC_API void mdc_trainer_destroy(mdc_trainer* t);

/* ---- head training: the dense layers of VT-CNN2 (or of any net that ends the same way) on precomputed feature rows --------
 * mdc_trainer_create refuses MDC_KIND_VTCNN2.  Of its 2,830,427 parameters 2,706,443 sit in dense1 (10,560 x 256) and dense2
 * (256 x C); with the two conv layers frozen no gradient flows back through the Flatten, and what is left to train is
 *     features (K) -> Dense(H, relu) -> Dense(C) -> softmax
 * over the rows that mdc_forward(..., MDC_TAP_FLAT) delivers at every dtype: transfer learning.  VT-CNN2 is (K, H, C) =
 * (10560, 256, C); the bounds are K a multiple of 32 in 32..16384, H a multiple of 32 in 32..256, C in 2..16.  f32.
 * Everything the "training" block above says holds here word for word unless stated otherwise: the loss (Keras 2.4's
 * categorical cross-entropy on the softmax OUTPUT, q = p / sum(p) clipped to [1e-7, 1 - 1e-7], mean over `count`; the clip
 * passes no gradient outside its interval, the ReLU none where z1 <= 0; target rows may be any distribution), TensorFlow 2.4's
 * Adam with its step count on the device, apply = 0, the MDC_TRAIN_* tensor kinds, the skipped-and-counted out-of-range index
 * that makes the next read return MDC_EINVAL, enqueue-only batches (no synchronisation, no allocation, no copy: capturable in a
 * hipGraph), bit-identical steps (fixed-order reductions, no float atomics -- also where the kernels split a batch over `count`
 * or over K), one stream at a time per trainer.
 * The training forward of one row f (feat_dev: f32 rows (n_rows, K), row-major, 16-byte aligned, the caller's device buffer):
 *     a = f * s0;  z1 = a W1 + b1;  h = relu(z1) * s1;  z2 = h W2 + b2;  p = softmax(z2)
 * with s0 = s1 = 1 unless Dropout is on (mdc_head_trainer_set_dropout): then each is keep / (1 - rate) from the generator that
 * mdc_trainer_set_dropout states, frame = the row's index in feat_dev, site 0 = the features (e = index in the row), site 1 =
 * the hidden units.  Backward: dW1 = a^T dz1, db1 = sum dz1, dW2 = h^T dz2, db2 = sum dz2; there is no feature gradient.
 * Evaluation has no Dropout; besides the loss sum and the row count it counts the rows whose arg-max of p equals the arg-max
 * of their target row (the lowest index on a tie, both sides).
 * Layer 0 is dense1 (kernel K x H, bias H), layer 1 dense2 (kernel H x C, bias C): Keras' (in, out) layouts.
 * A training batch is five launches (Z1 partial products, the row kernel, dW1 partial products, the small gradients, reduce +
 * Adam) and, with apply != 0, a one-thread sixth that advances the step count; an evaluation is three. */
typedef struct mdc_head_trainer mdc_head_trainer;   /* opaque: f32 master weights, Adam state, all scratch for max_batch rows */

/* All device memory is allocated here; 1 <= max_batch <= 65536 bounds `count` of every later call. */
MDC_API int mdc_head_trainer_create(int features, int hidden, int classes, int64_t max_batch, int device, mdc_head_trainer** out);
MDC_API int mdc_head_trainer_set_adam(mdc_head_trainer* t, float lr, float beta1, float beta2, float eps);
/* Dropout(rate_features) in front of dense1 and Dropout(rate_hidden) behind it, each in [0, 1); 0 = off (the default). */
MDC_API int mdc_head_trainer_set_dropout(mdc_head_trainer* t, float rate_features, float rate_hidden, uint32_t seed);
MDC_API int mdc_head_trainer_set_tensor(mdc_head_trainer* t, int which, int layer, const float* kernel_host, size_t kernel_elems,
                                const float* bias_host, size_t bias_elems, void* hip_stream);
MDC_API int mdc_head_trainer_get_tensor(mdc_head_trainer* t, int which, int layer, float* kernel_host, size_t kernel_elems,
                                float* bias_host, size_t bias_elems, void* hip_stream);
MDC_API int mdc_head_trainer_set_iterations(mdc_head_trainer* t, int64_t iterations, void* hip_stream);
/* One step on the rows order_dev[first .. first + count) of (feat_dev, y_dev); y_dev: f32 target rows (n_rows, C).
 * count <= max_batch.  A batch before both layers' MDC_TRAIN_WEIGHTS are set is MDC_ESTATE. */
MDC_API int mdc_head_train_batch(mdc_head_trainer* t, const float* feat_dev, const float* y_dev, int64_t n_rows, const int32_t* order_dev,
                         int64_t first, int64_t count, int apply, void* hip_stream);
MDC_API int mdc_head_trainer_evaluate(mdc_head_trainer* t, const float* feat_dev, const float* y_dev, int64_t n_rows, const int32_t* order_dev,
                              int64_t first, int64_t count, void* hip_stream);
/* As mdc_trainer_read, plus eval_correct; reset != 0 zeroes the five statistics (not `iterations`). */
MDC_API int mdc_head_trainer_read(mdc_head_trainer* t, int reset, double* train_loss_sum, int64_t* train_rows, double* eval_loss_sum,
                          int64_t* eval_rows, int64_t* eval_correct, int64_t* iterations, void* hip_stream);
MDC_API void mdc_head_trainer_destroy(mdc_head_trainer* t);

MDC_API const char* mdc_last_error(void);
MDC_API void mdc_destroy(mdc_model* m);

#ifdef __cplusplus
}
#endif
#endif /* MDC_H */
