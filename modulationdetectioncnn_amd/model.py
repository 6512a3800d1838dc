"""Host-side mirror of the reference's Keras surface for the inference path.

    reference (cnn.py / CNN.ipynb)                     here
    -----------------------------------------------    -----------------------------------
    model = models.Sequential(); model.add(...)        m = VTCNN2(Topology.deployed(3))
    model.load_weights(filepath)      cnn.py:147       m.load_weights(path)   (.h5 | .txt | .npz)
    model.compile(loss=..., optimizer='adam') :113     m.compile(loss='categorical_crossentropy', optimizer='adam')
    history = model.fit(X, Y, ...)    cnn.py:135       history = m.fit(X, Y, batch_size=1024, epochs=100, validation_data=...,
                                                                       checkpoint=filepath, patience=5)   (training.py)
    model.predict(X, batch_size=1024) cnn.py:198       m.predict(X, batch_size=1024)
    int(np.argmax(Y_hat[i,:]))        cnn.py:209       m.predict_classes(X)
    Model(inputs, layers[i].output)   CNN.ipynb c.17   m.predict(X, tap='conv'|'flat'|'dense'), or the cell's own spelling:
                                                       Model(inputs=m.inputs, outputs=m.layers[4].output).predict(X)

All arithmetic runs in libmdc.so (hand-written gfx950 HIP) through the C ABI in
include/mdc.h; PyTorch-ROCm only supplies device memory and the HIP stream.  numpy in ->
numpy out (PCIe-bound plumbing); torch-ROCm tensor in -> torch tensor out on the same device,
enqueued on torch's current stream with no synchronisation.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _cabi
from .formats import q612
from .formats.h5mini import load_keras_h5
from .topology import Topology, synthetic_weights

_KIND = {"deployed": _cabi.KIND_DEPLOYED, "vtcnn2": _cabi.KIND_VTCNN2, "cnnpy": _cabi.KIND_CNNPY}
_DTYPE = {"f32": _cabi.F32, "fp32": _cabi.F32, "float32": _cabi.F32, "bf16": _cabi.BF16, "bfloat16": _cabi.BF16,
          "fp8": _cabi.FP8, "f16": _cabi.F16, "fp16": _cabi.F16, "float16": _cabi.F16}
# slots of the host-buffer driver are at least this long (frames), whatever batch_size a Keras-style call passes
HOST_MIN_CHUNK = 16384

_TAP = {None: _cabi.TAP_NONE, "conv": _cabi.TAP_CONV, "flat": _cabi.TAP_FLAT, "dense": _cabi.TAP_DENSE,
        "hidden": _cabi.TAP_HIDDEN}

Weights = List[Tuple[np.ndarray, np.ndarray]]

# nonfinite= of the inference calls: None = mdc_forward / mdc_predict_host as they are; otherwise the checked entry points
# (include/mdc.h, "non-finite input frames") with this policy
_NONFINITE = {"propagate": _cabi.NONFINITE_PROPAGATE, "raise": _cabi.NONFINITE_REPORT}


class NonFiniteInputError(ValueError):
    """nonfinite="raise": some input frames hold a NaN or +-Inf sample.  .frames: their indices (sorted), .count: how many."""

    def __init__(self, frames: Sequence[int]):
        self.frames = [int(i) for i in frames]
        self.count = len(self.frames)
        shown = ", ".join(str(i) for i in self.frames[:8]) + (", ..." if self.count > 8 else "")
        super().__init__(f"{self.count} input frame(s) hold a NaN or +-Inf sample: {shown}")


def _nonfinite_policy(nonfinite: Optional[str], tap: Optional[str] = None) -> Optional[int]:
    if nonfinite is None:
        return None
    if nonfinite not in _NONFINITE:
        raise ValueError(f"nonfinite must be None, 'propagate' or 'raise'; got {nonfinite!r}")
    if tap is not None:
        raise ValueError("nonfinite= and tap= cannot be combined: the checked forward has no layer taps")
    return _NONFINITE[nonfinite]


def _torch():
    import torch
    return torch


class VTCNN2:
    """A VT-CNN2-family classifier bound to one MI355X."""

    # scratch buffers kept alive at once (one per stream that forwards concurrently; least recently used goes first)
    MAX_WORKSPACES = 4

    def __init__(self, topology: Topology, device: Union[int, str, None] = None, dtype: str = "f32",
                 fp8_input_absmax: Optional[float] = None, fp8_bf16_features: bool = False,
                 fp8_feature_absmax: Optional[float] = None, _lib_variant: str = "product"):
        """dtype "f32" | "bf16" (vtcnn2, deployed) | "f16" (deployed) | "fp8" (vtcnn2, deployed).  fp8_input_absmax: the largest
        |I/Q sample| the fp8 mode must represent (default 0.02, the scale of the reference's frames); larger inputs saturate.
        fp8_bf16_features (vtcnn2 at "fp8" only): MDC_OPT_FP8_BF16_FEATURES -- keep the conv2 features in bf16 as before
        ABI 4 instead of E4M3 bytes (twice the feature traffic, the old numerics).
        fp8_feature_absmax (vtcnn2 at "fp8", E4M3 features): the largest conv2 feature to represent (mdc_set_fp8_feature_absmax);
        None = the library's estimate from the weights; calibrate_fp8_features() measures it on a sample.
        _lib_variant: tests only (the alternates build)."""
        self.topology = topology
        self.dtype = dtype
        self.fp8_input_absmax = fp8_input_absmax
        self.fp8_bf16_features = bool(fp8_bf16_features)
        self._fp8_feature_absmax = fp8_feature_absmax
        if self.fp8_bf16_features and not (topology.kind == "vtcnn2" and dtype == "fp8"):
            raise ValueError("fp8_bf16_features is an option of the vtcnn2 family's fp8 mode")
        self._lib_variant = _lib_variant
        if dtype not in _DTYPE:
            raise ValueError(f"dtype must be one of {sorted(_DTYPE)}")
        # the device is resolved ONCE (None = the device current at construction): the engine handle, the workspace
        # and the input check all use this stored ordinal, whatever torch.cuda.set_device() does later
        self._device_index: Optional[int] = self._resolve_device(device)
        self._weights: Optional[Weights] = None
        self._handle: Optional[C.c_void_p] = None
        self._ws = {}
        self._ws_captured = []  # buffers whose address a captured hipGraph holds (never evicted; see _workspace)
        self._ws_need = {}      # frames per launch -> mdc_workspace_bytes (a property of the finalized model)
        # frames per mdc_forward call when the caller gives no batch_size.  VT-CNN2: the workspace holds one call's features
        # (21.6 KB/frame in the 16-bit modes, 42 KB at f32): 65,536 frames per call = 1.45 GB (f32: 2.8 GB) per stream, and
        # every launch still fills the chip 16 times over.  A caller with HBM to spare passes batch_size=1 << 20 (23 GB of
        # workspace, +1.5 %: one launch of each kernel instead of sixteen) -- bench.py's headline does, and says so.
        self.default_chunk = 1 << 16 if topology.kind == "vtcnn2" else 1 << 22

    # what the packed engine was built from cannot change under it
    _FIXED = ("topology", "dtype", "fp8_bf16_features", "_lib_variant")

    def __setattr__(self, name, value):
        if name in VTCNN2._FIXED and name in self.__dict__:
            raise AttributeError(f"{name} is fixed at construction: build another VTCNN2")
        if name == "fp8_input_absmax" and self.__dict__.get("_handle") is not None:
            self._release()                 # re-packed with the new activation scale at the next use
        object.__setattr__(self, name, value)

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_h5(cls, path: str, **kw) -> "VTCNN2":
        ck = load_keras_h5(path)
        m = cls(Topology.from_keras_config(ck.model_config), **kw)
        m._set_from_checkpoint(ck)
        return m

    @classmethod
    def from_npz(cls, path: str, **kw) -> "VTCNN2":
        """Decoded-weights fixture (tests/golden/weights/*.npz, made by tools/make_golden.py)."""
        z = np.load(path)
        F = int(z["conv_bias"].shape[0])
        m = cls(Topology.deployed(F, int(z["dense_bias"].shape[0])), **kw)
        m.set_weights([(z["conv_kernel"], z["conv_bias"]), (z["dense_kernel"], z["dense_bias"])])
        return m

    @classmethod
    def from_txt(cls, path: str, conv_from: Optional[str] = None, strict: bool = False, **kw) -> "VTCNN2":
        """Q6.12 text export.  F=10 dumps hold only the dense kernel: ``conv_from`` names the .h5
        (or .npz fixture) supplying conv kernel/bias and dense bias."""
        w = q612.load_weights_txt(path, strict=strict)
        m = cls(Topology.deployed(w.filters, 3), **kw)
        donor = None
        if conv_from is not None:
            donor = (cls.from_npz(conv_from) if conv_from.endswith(".npz") else cls.from_h5(conv_from))._weights
        parts = {"conv_kernel": w.conv_kernel, "conv_bias": w.conv_bias, "dense_kernel": w.dense_kernel, "dense_bias": w.dense_bias}
        if w.placeholder_dense:
            parts["dense_kernel"] = None      # 12.14.weights.txt: six identical placeholder tables
        if donor is not None:
            fill = {"conv_kernel": donor[0][0], "conv_bias": donor[0][1], "dense_kernel": donor[1][0], "dense_bias": donor[1][1]}
            for k, v in fill.items():
                if parts[k] is None:
                    parts[k] = v
        missing = [k for k, v in parts.items() if v is None]
        if missing:
            raise ValueError(f"{os.path.basename(path)} lacks {missing}; pass conv_from=<.h5 or .npz>")
        m.set_weights([(parts["conv_kernel"], parts["conv_bias"]), (parts["dense_kernel"], parts["dense_bias"])])
        return m

    @classmethod
    def synthetic(cls, topology: Union[Topology, str] = "vtcnn2", classes: int = 11, seed: int = 2016,
                  bias_scale: float = 0.0, **kw) -> "VTCNN2":
        if isinstance(topology, str):
            topology = {"vtcnn2": Topology.vtcnn2(classes), "deployed3": Topology.deployed(3, 3),
                        "deployed10": Topology.deployed(10, 3), "cnnpy": Topology.cnnpy(10, 10, classes)}[topology]
        m = cls(topology, **kw)
        m.set_weights(synthetic_weights(topology, seed, bias_scale))
        return m

    # ------------------------------------------------------------------ weights
    def _set_from_checkpoint(self, ck) -> None:
        tensors = [a for l in ck.layer_names for _, a in ck.weights[l]]
        if len(tensors) != 2 * len(self.topology.layer_shapes):
            raise ValueError(f"{ck.path}: {len(tensors)} tensors for {len(self.topology.layer_shapes)} weighted layers")
        self.set_weights([(tensors[2 * i], tensors[2 * i + 1]) for i in range(len(tensors) // 2)])

    def load_weights(self, filepath: str, conv_from: Optional[str] = None) -> None:
        """``model.load_weights(filepath)`` (cnn.py:147): topology must match the file's."""
        if filepath.endswith((".h5", ".hdf5")):
            ck = load_keras_h5(filepath)
            t = Topology.from_keras_config(ck.model_config)
            if t != self.topology:
                raise ValueError(f"{filepath} holds {t}, model is {self.topology}")
            self._set_from_checkpoint(ck)
        elif filepath.endswith(".npz"):
            self.set_weights(VTCNN2.from_npz(filepath)._weights)
        elif filepath.endswith(".txt"):
            self.set_weights(VTCNN2.from_txt(filepath, conv_from=conv_from)._weights)
        else:
            raise ValueError(f"unknown weight file type: {filepath}")

    def set_weights(self, weights: Sequence[Tuple[np.ndarray, np.ndarray]], theano_kernels: bool = False) -> None:
        """[(kernel, bias)] per weighted layer in the layouts of `Topology.layer_shapes`.  The kernels are applied as
        Keras-2/TensorFlow applies them: cross-correlation.  `theano_kernels=True` is for a checkpoint trained with
        Keras 1 on the Theano backend, as the vendored DeepSig notebook was (RML2016.10a_VTCNN2_example.ipynb:229-243
        under `K.set_image_dim_ordering('th')`): Theano's conv2d CONVOLVES, i.e. applies each filter flipped along both
        spatial axes, so the 4-D kernels are flipped once here and everything below stays a correlation."""
        shapes = self.topology.layer_shapes
        if len(weights) != len(shapes):
            raise ValueError(f"expected {len(shapes)} (kernel, bias) pairs, got {len(weights)}")
        out = []
        for i, ((k, b), (ks, bs)) in enumerate(zip(weights, shapes)):
            k = np.ascontiguousarray(k, dtype=np.float32)
            b = np.ascontiguousarray(b, dtype=np.float32)
            if theano_kernels and k.ndim == 4:
                sp = (2, 3) if self.topology.kind == "vtcnn2" else (0, 1)      # OIHW / HWIO: the two spatial axes
                k = np.ascontiguousarray(np.flip(k, axis=sp))
            if tuple(k.shape) != ks or tuple(b.shape) != bs:
                raise ValueError(f"layer {i} ({self.topology.layer_names[i]}): expected kernel {ks} bias {bs}, got {k.shape} {b.shape}")
            out.append((k, b))
        self._weights = out
        self._release()
        t = getattr(self, "_trainer", None)
        if t is not None:           # as in Keras: set_weights / load_weights replace the layers' variables, the optimizer keeps its
            t.set_weights(out)      # slots (Adam's m, v, iterations) -- cnn.py:147 reloads the best epoch into a compiled model

    def get_weights(self) -> Weights:
        if self._weights is None:
            raise RuntimeError("no weights loaded")
        return [(k.copy(), b.copy()) for k, b in self._weights]

    # ------------------------------------------------------------------ training (cnn.py:113, 122-147)
    def compile(self, loss: str = "categorical_crossentropy", optimizer: str = "adam", lr: float = 1e-3, beta1: float = 0.9,
                beta2: float = 0.999, eps: float = 1e-7, dropout: float = 0.0, dropout_seed: int = 0) -> None:
        """``model.compile(loss='categorical_crossentropy', optimizer='adam')`` (cnn.py:113): the one loss and the one
        optimizer the reference uses; the keyword arguments are keras.optimizers.Adam's (its defaults).  dropout: the optional
        Dropout(dr) of the DeepSig definition behind the conv activations (training batches only; 0 = the reference's nets)."""
        if loss != "categorical_crossentropy" or str(optimizer).lower() != "adam":
            raise ValueError("the reference compiles with loss='categorical_crossentropy', optimizer='adam'; nothing else is built")
        self._adam = dict(lr=float(lr), beta1=float(beta1), beta2=float(beta2), eps=float(eps), dropout=float(dropout),
                          dropout_seed=int(dropout_seed))
        self._drop_trainer()

    def _drop_trainer(self) -> None:
        t = getattr(self, "_trainer", None)
        if t is not None:
            t.close()
        self._trainer = None

    def trainer(self):
        """The training state behind fit(): created on first use from the current weights; it lives on (as a compiled Keras
        model's optimizer does) until the weights are replaced from outside."""
        from .training import Trainer
        if getattr(self, "_trainer", None) is None:
            if self._weights is None:
                raise RuntimeError("set or load weights (or VTCNN2.synthetic) before fit()")
            self._trainer = Trainer(self.topology, self._weights, device=self.device_index, _lib_variant=self._lib_variant,
                                    **getattr(self, "_adam", {}))
        return self._trainer

    def fit(self, X, Y, batch_size: int = 1024, epochs: int = 100, validation_data=None, patience: Optional[int] = 5,
            checkpoint: Optional[str] = None, shuffle: bool = True, seed: Optional[int] = None, verbose: int = 0, **kw):
        """``model.fit(X_train, Y_train, batch_size, epochs, validation_data=(X_test, Y_test), callbacks=[ModelCheckpoint(
        checkpoint, monitor='val_loss', save_best_only=True), EarlyStopping(monitor='val_loss', patience=patience)])``
        (cnn.py:135-146; ``callbacks=[...]`` with the two classes of ``modulationdetectioncnn_amd.callbacks`` is accepted
        verbatim) for the deployed and cnn.py nets, f32, on the MI355X (csrc/train.hip).  As in Keras the model is
        left with the LAST epoch's weights; the best ones are in `checkpoint` (a Keras full-model .h5: ``load_weights`` it,
        as cnn.py:147 does) and in the returned history's ``best_weights``."""
        t = self.trainer()
        hist = t.fit(X, Y, batch_size=batch_size, epochs=epochs, validation_data=validation_data, patience=patience,
                     checkpoint=checkpoint, shuffle=shuffle, seed=seed, verbose=verbose, **kw)
        self._weights = t.get_weights()
        self._release()                     # the inference engine re-packs the new weights on its next use
        return hist

    def save(self, filepath: str) -> None:
        """``model.save(filepath)``: Keras 2.4 full-model HDF5 (formats/h5mini.write_keras_h5); Adam's state is included when
        this model has been fitted."""
        from .formats.h5mini import write_keras_h5
        if self._weights is None:
            raise RuntimeError("no weights loaded")
        t = getattr(self, "_trainer", None)
        write_keras_h5(filepath, self.topology, self._weights, optimizer=t.optimizer_state() if t is not None else None,
                       adam={k: v for k, v in (getattr(self, "_adam", None) or {}).items() if not k.startswith("dropout")})

    # ------------------------------------------------------------------ engine
    def _lib(self):
        return _cabi.lib(self._lib_variant)

    def _check(self, rc: int) -> int:
        return _cabi.check(rc, self._lib_variant)

    @staticmethod
    def _resolve_device(device) -> Optional[int]:
        """int | "cuda:N" | torch.device | None.  None is resolved when a GPU is present (at construction, else at
        first use: models are also built on GPU-less hosts to read or convert weights)."""
        if isinstance(device, (int, np.integer)):
            return int(device)
        torch = _torch()
        if device is None:
            return torch.cuda.current_device() if torch.cuda.is_available() else None
        d = torch.device(device)
        if d.type != "cuda":
            raise ValueError(f"the MI355X path needs a cuda (ROCm) device, got {device!r}")
        return d.index if d.index is not None else (torch.cuda.current_device() if torch.cuda.is_available() else None)

    @property
    def device_index(self) -> int:
        if self._device_index is None:
            self._device_index = _torch().cuda.current_device()
        return self._device_index

    def _engine(self) -> C.c_void_p:
        if self._handle is not None:
            return self._handle
        if self._weights is None:
            raise RuntimeError("load_weights() before predict()")
        torch = _torch()
        if not torch.cuda.is_available():
            raise RuntimeError("no ROCm device visible: the MI355X path has no CPU fallback")
        L = self._lib()
        t = self.topology
        topo = _cabi.MdcTopology(_KIND[t.kind], t.filters, t.hidden, t.classes,
                                 (C.c_int32 * 4)(_cabi.MDC_OPT_FP8_BF16_FEATURES if self.fp8_bf16_features else 0, 0, 0, 0))
        h = C.c_void_p()
        self._check(L.mdc_create(C.byref(topo), self.device_index, C.byref(h)))
        try:
            for i, (k, b) in enumerate(self._weights):
                self._check(L.mdc_set_weights(h, i, k.ctypes.data_as(C.POINTER(C.c_float)), k.size,
                                              b.ctypes.data_as(C.POINTER(C.c_float)), b.size))
            if self.fp8_input_absmax is not None:
                self._check(L.mdc_set_fp8_input_absmax(h, float(self.fp8_input_absmax)))
            if self.fp8_feature_absmax is not None and t.kind == "vtcnn2" and self.dtype == "fp8" and not self.fp8_bf16_features:
                self._check(L.mdc_set_fp8_feature_absmax(h, float(self.fp8_feature_absmax)))
            self._check(L.mdc_finalize(h, _DTYPE[self.dtype]))
        except Exception:
            L.mdc_destroy(h)
            raise
        self._handle = h
        return h

    @property
    def fp8_feature_absmax(self) -> Optional[float]:
        """The caller's bound on the conv2 features for the E4M3 feature scale (None: the estimate from the weights).  Setting it
        re-packs the engine at its next use."""
        return self._fp8_feature_absmax

    @fp8_feature_absmax.setter
    def fp8_feature_absmax(self, value: Optional[float]) -> None:
        if value is not None and not float(value) > 0.0:
            raise ValueError("fp8_feature_absmax must be positive (or None)")
        self._fp8_feature_absmax = None if value is None else float(value)
        if getattr(self, "_handle", None) is not None:
            self._release()

    def calibrate_fp8_features(self, X, headroom: float = 2.0) -> float:
        """Calibration of the fp8 mode's E4M3 feature scale on a sample batch: the same weights in bf16 mode, the
        conv tap of X, `headroom` x its largest value -> mdc_set_fp8_feature_absmax at the next (re-)finalize.  Returns the
        value set.  X: a few hundred representative frames."""
        if not (self.topology.kind == "vtcnn2" and self.dtype == "fp8" and not self.fp8_bf16_features):
            raise ValueError("calibration applies to the vtcnn2 family's fp8 mode with E4M3 features")
        probe = VTCNN2(self.topology, device=self.device_index, dtype="bf16", _lib_variant=self._lib_variant)
        probe.set_weights(self._weights)
        top = float(np.asarray(probe.predict(np.asarray(X, np.float32), tap="conv")).max())
        probe._release()
        if not top > 0.0:
            raise ValueError("the sample produced no positive conv2 feature")
        self.fp8_feature_absmax = headroom * top      # (the setter releases the packed engine)
        return self.fp8_feature_absmax

    def _release(self) -> None:
        if self._handle is not None:
            self._lib().mdc_destroy(self._handle)
            self._handle = None
        self._ws = {}
        self._ws_captured = []
        self._ws_need = {}

    def __del__(self):
        try:
            self._release()
            self._drop_trainer()
        except Exception:
            pass

    def _workspace(self, n: int, stream_key: Optional[int] = None):
        need = self._ws_need.get(n)
        if need is None:
            need = self._ws_need[n] = int(self._lib().mdc_workspace_bytes(self._engine(), n))
        if need == 0:
            return None, 0
        torch = _torch()
        # one scratch buffer PER STREAM: forwards enqueued on different streams run concurrently and must not share
        # it (the C ABI leaves the workspace to the caller for exactly this reason); allocated under the stream
        # that uses it, so torch's caching allocator orders any reuse after the launches already queued there
        key = stream_key if stream_key is not None else torch.cuda.current_stream(torch.device("cuda", self.device_index)).cuda_stream
        ws = self._ws.pop(key, None)
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=f"cuda:{self.device_index}")
        self._ws[key] = ws                      # (dict order = recency: re-inserted at the end)
        if torch.cuda.is_current_stream_capturing() and not any(w is ws for w in self._ws_captured):
            # a hipGraph being captured bakes this buffer's ADDRESS into its kernel nodes: the buffer must outlive every
            # replay, so neither the LRU below nor a later, larger chunk may hand it back to the allocator.
            # It stays referenced here until release_captured_workspaces() / the model goes away.
            self._ws_captured.append(ws)
        while len(self._ws) > self.MAX_WORKSPACES:
            # streams that are gone (worker threads' streams, a finished MultiStreamPredictor) do not pin HBM for ever:
            # the least recently used buffer goes back to torch's caching allocator, which keeps a block freed while
            # its stream still has work queued away from other streams until that work is done
            self._ws.pop(next(iter(self._ws)))
        return ws, need

    def reserve_workspace(self, frames_per_call: int) -> int:
        """Allocate (now, on torch's current stream) the scratch buffer a forward of `frames_per_call` frames per
        mdc_forward call needs, so that the first timed / captured forward allocates nothing; returns its bytes."""
        _ws, need = self._workspace(int(frames_per_call))
        return need

    def release_captured_workspaces(self) -> None:
        """Drop the references that keep scratch buffers alive for captured hipGraphs.  Call only after every graph
        captured from this model's forwards has been destroyed: a replay after this writes through a stale address."""
        self._ws_captured = []

    def build(self, input_shape=None) -> None:
        """``model.build()`` (cnn.py:114): the topology fixes every shape already."""

    def summary(self) -> None:
        """``model.summary()`` (cnn.py:115) prints the layer table."""
        print(self.topology.summary())

    # ------------------------------------------------------------------ model.layers / model.inputs (CNN.ipynb cells 15, 17)
    @property
    def layers(self) -> List["Layer"]:
        """The Sequential's layers in Keras' order (`print(model.layers[2])`, `model.layers[4].output`: CNN.ipynb cells 15, 17)."""
        rows = self.topology.keras_layers()
        names = self.topology.keras_layer_names()
        return [Layer(self, i, cls, name, shape, params) for i, ((cls, shape, params), (_role, name)) in enumerate(zip(rows, names))]

    @property
    def inputs(self) -> "ModelInputs":
        return ModelInputs(self)

    # ------------------------------------------------------------------ inference
    def tap_shape(self, tap: str) -> Tuple[int, ...]:
        t = self.topology
        if t.kind == "deployed":
            return {"conv": (2, 129, t.filters), "flat": (258 * t.filters,), "dense": (t.classes,)}[tap]
        if t.kind == "vtcnn2":
            return {"conv": (80, 132), "flat": (10560,), "dense": (t.classes,), "hidden": (256,)}[tap]
        return {"conv": (1, 3, t.filters), "flat": (3 * t.filters,), "dense": (t.classes,), "hidden": (t.hidden,)}[tap]

    def forward_device(self, x, probs=None, labels=None, tap: Optional[str] = None, tap_out=None,
                       batch_size: Optional[int] = None, nonfinite: Optional[str] = None, nonfinite_out=None):
        """Enqueue the forward on torch's current stream.  x: contiguous float32 CUDA tensor (n,2,128).
        Pre-allocated outputs may be passed; returns (probs, labels, tap_out).
        nonfinite="propagate" | "raise" (mdc_forward_checked, no taps; tap_out stays None): the (n,) uint8 per-frame flags
        (1 = the frame holds a NaN or +-Inf sample) go to nonfinite_out, a caller's tensor, if given.  "propagate": flagged frames
        get an all-NaN row and label 0, as Keras' predict + np.argmax give them.  "raise": the results are mdc_forward's,
        and if any frame is flagged the call synchronises and raises NonFiniteInputError (the count is read back always,
        the flags only then)."""
        policy = _nonfinite_policy(nonfinite, tap)
        if nonfinite_out is not None and policy is None:
            raise ValueError("nonfinite_out needs nonfinite='propagate' or 'raise'")
        torch = _torch()
        if not (isinstance(x, torch.Tensor) and x.is_cuda):
            raise TypeError("forward_device needs a torch tensor on the ROCm device")
        if x.dtype != torch.float32 or tuple(x.shape[1:]) != (2, 128) or not x.is_contiguous():
            raise ValueError(f"input must be contiguous float32 (n,2,128); got {x.dtype} {tuple(x.shape)}")
        if x.device.index != self.device_index:
            raise ValueError(f"input on cuda:{x.device.index}, model on cuda:{self.device_index}")
        if tap not in _TAP:
            raise ValueError(f"tap must be one of {[k for k in _TAP if k]}")
        n = x.shape[0]
        Cn = self.topology.classes
        h = self._engine()
        L = self._lib()
        dev = x.device
        if probs is None:
            probs = torch.empty((n, Cn), dtype=torch.float32, device=dev)
        if labels is None:
            labels = torch.empty((n,), dtype=torch.int32, device=dev)
        if tap is not None and tap_out is None:
            tap_out = torch.empty((n,) + self.tap_shape(tap), dtype=torch.float32, device=dev)
        if policy is not None:
            if nonfinite_out is None:
                nonfinite_out = torch.empty((n,), dtype=torch.uint8, device=dev)
            elif not (isinstance(nonfinite_out, torch.Tensor) and nonfinite_out.dtype == torch.uint8 and tuple(nonfinite_out.shape) == (n,)
                      and nonfinite_out.is_contiguous() and nonfinite_out.device == dev):
                raise ValueError(f"nonfinite_out must be a contiguous uint8 tensor of shape ({n},) on {dev}")
        if n == 0:
            return probs, labels, tap_out
        chunk = int(batch_size) if batch_size else self.default_chunk
        chunk = max(1, min(chunk, n))
        stream = torch.cuda.current_stream(dev).cuda_stream      # (2 us: looked up once per call)
        ws, ws_bytes = self._workspace(chunk, stream)
        tap_row = int(np.prod(self.tap_shape(tap))) if tap is not None else 0
        if policy is not None:
            count = torch.zeros((1,), dtype=torch.int64, device=dev) if nonfinite == "raise" else None
            for s in range(0, n, chunk):
                m = min(chunk, n - s)
                self._check(L.mdc_forward_checked(
                    h, x.data_ptr() + s * 1024, m, probs.data_ptr() + s * Cn * 4, labels.data_ptr() + s * 4,
                    ws.data_ptr() if ws is not None else None, ws_bytes, nonfinite_out.data_ptr() + s,
                    count.data_ptr() if count is not None else None, policy, stream))
            if count is not None and int(count.item()):
                raise NonFiniteInputError(torch.nonzero(nonfinite_out).flatten().tolist())
            return probs, labels, None
        for s in range(0, n, chunk):
            m = min(chunk, n - s)
            self._check(L.mdc_forward(
                h, x.data_ptr() + s * 1024, m,
                probs.data_ptr() + s * Cn * 4, labels.data_ptr() + s * 4,
                (tap_out.data_ptr() + s * tap_row * 4) if tap is not None else None, _TAP[tap],
                ws.data_ptr() if ws is not None else None, ws_bytes, stream))
        return probs, labels, tap_out

    def _host_chunk(self, batch_size) -> int:
        """Keras' batch_size is a speed knob, not a result knob (results do not depend on it): the host-buffer driver
        keeps its slots at least HOST_MIN_CHUNK frames long, whatever the caller's cnn.py:198 passes (1024 there)."""
        return max(int(batch_size), HOST_MIN_CHUNK) if batch_size else 0

    def predict_host(self, X: np.ndarray, batch_size: Optional[int] = None, want_probs: bool = True,
                     want_labels: bool = True, out=None, nonfinite: Optional[str] = None) -> Tuple[Optional[np.ndarray], Optional[np.ndarray]]:
        """numpy frames in, numpy (probs, labels) out through the library's own host-buffer driver (mdc_predict_host:
        pinned ring, copy / compute / result streams overlapped).  Bit-identical to the device path.  out = (probs,
        labels): write into the caller's C-contiguous float32 (n,C) / int32 (n,) arrays (slices of a larger batch's).
        nonfinite="propagate" | "raise": mdc_predict_host_checked, as forward_device describes."""
        policy = _nonfinite_policy(nonfinite)
        a = np.ascontiguousarray(np.asarray(X), dtype=np.float32)
        if a.ndim != 3 or a.shape[1:] != (2, 128):
            raise ValueError(f"expected input of shape (n,2,128); got {a.shape}")
        n, Cn = a.shape[0], self.topology.classes
        if out is not None:
            probs, labels = out
            for arr, shape, dt in ((probs, (n, Cn), np.float32), (labels, (n,), np.int32)):
                if arr is not None and not (isinstance(arr, np.ndarray) and arr.shape == shape and arr.dtype == dt and arr.flags.c_contiguous
                                            and arr.flags.writeable):
                    raise ValueError(f"out arrays must be writeable C-contiguous {np.dtype(dt).name} of shape {shape}")
        else:
            probs = np.empty((n, Cn), np.float32) if want_probs else None
            labels = np.empty((n,), np.int32) if want_labels else None
        if policy is not None:
            flags = np.empty((n,), np.uint8)
            count = C.c_int64(0)
            self._check(self._lib().mdc_predict_host_checked(self._engine(), a.ctypes.data, n,
                                                             probs.ctypes.data if probs is not None else None,
                                                             labels.ctypes.data if labels is not None else None, flags.ctypes.data,
                                                             C.byref(count), policy, self._host_chunk(batch_size)))
            if nonfinite == "raise" and count.value:
                raise NonFiniteInputError(np.flatnonzero(flags).tolist())
            return probs, labels
        self._check(self._lib().mdc_predict_host(self._engine(), a.ctypes.data, n,
                                                 probs.ctypes.data if probs is not None else None,
                                                 labels.ctypes.data if labels is not None else None, self._host_chunk(batch_size)))
        return probs, labels

    def _run(self, X, batch_size, tap, nonfinite=None):
        torch = _torch()
        as_numpy = not isinstance(X, torch.Tensor)
        if as_numpy:
            a = np.ascontiguousarray(np.asarray(X), dtype=np.float32)
            if a.ndim != 3 or a.shape[1:] != (2, 128):
                raise ValueError(f"expected input of shape (n,2,128); got {a.shape}")
            x = torch.from_numpy(a).to(f"cuda:{self.device_index}")
        else:
            x = X
            if not x.is_cuda:
                x = x.to(f"cuda:{self.device_index}")
            x = x.to(torch.float32).contiguous()
        probs, labels, tap_out = self.forward_device(x, tap=tap, batch_size=batch_size, nonfinite=nonfinite)
        return as_numpy, probs, labels, tap_out

    def predict(self, X, batch_size: Optional[int] = None, tap: Optional[str] = None, verbose: int = 0, nonfinite: Optional[str] = None):
        """``model.predict(X, batch_size)``: (n,C) float32 softmax rows (``verbose`` is accepted and says nothing); with ``tap`` the named
        intermediate layer of CNN.ipynb cell 17 instead.  Results do not depend on batch_size.  numpy in -> numpy out
        (through the streaming host-buffer driver); torch-ROCm tensor in -> tensor out on torch's current stream.
        nonfinite="propagate": frames holding a NaN / +-Inf sample get Keras' all-NaN row; "raise": NonFiniteInputError
        names them (see forward_device)."""
        _nonfinite_policy(nonfinite, tap)
        if tap is None and not isinstance(X, _torch().Tensor):
            return self.predict_host(X, batch_size, want_labels=False, nonfinite=nonfinite)[0]
        as_numpy, probs, _labels, tap_out = self._run(X, batch_size, tap, nonfinite)
        out = tap_out if tap is not None else probs
        return out.cpu().numpy() if as_numpy else out

    def predict_classes(self, X, batch_size: Optional[int] = None, nonfinite: Optional[str] = None):
        """Row-wise ``np.argmax`` of predict(X) (cnn.py:209: first maximum wins), int32 (n,).  nonfinite: as predict (a NaN
        row's argmax is 0)."""
        _nonfinite_policy(nonfinite)
        if not isinstance(X, _torch().Tensor):
            return self.predict_host(X, batch_size, want_probs=False, nonfinite=nonfinite)[1]
        as_numpy, _probs, labels, _ = self._run(X, batch_size, None, nonfinite)
        return labels.cpu().numpy() if as_numpy else labels

    # ------------------------------------------------------------------ evaluation (cnn.py:198-216)
    def confusion_counts_device(self, X, labels_true, batch_size: Optional[int] = None):
        """Un-normalised C x C counts ``conf[true, predicted]`` (cnn.py:205-216) as an int64 CUDA tensor, computed
        on the device (mdc_confusion); labels outside [0,C) raise."""
        torch = _torch()
        pred = self.predict_classes(X if isinstance(X, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(np.asarray(X), dtype=np.float32)).to(f"cuda:{self.device_index}"), batch_size)
        dev = pred.device
        truth = torch.as_tensor(np.asarray(labels_true) if not isinstance(labels_true, torch.Tensor) else labels_true)
        truth = truth.to(device=dev, dtype=torch.int32).contiguous()
        if truth.shape != pred.shape:
            raise ValueError(f"labels_true has shape {tuple(truth.shape)}, predictions {tuple(pred.shape)}")
        Cn = self.topology.classes
        counts = torch.zeros((Cn, Cn), dtype=torch.int64, device=dev)
        bad = torch.zeros((1,), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            self._check(self._lib().mdc_confusion(truth.data_ptr(), pred.data_ptr(), pred.numel(), Cn, counts.data_ptr(),
                                                  bad.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        nbad = int(bad.item())                  # the one synchronising read
        if nbad:
            raise ValueError(f"{nbad} labels lie outside [0, {Cn})")
        return counts

    def evaluate(self, X, Y, batch_size: Optional[int] = None, verbose: int = 0, nonfinite: Optional[str] = None) -> float:
        """``score = model.evaluate(X_test, Y_test, verbose=0, batch_size=...)`` (cnn.py:153): the reference compiles its model with
        loss='categorical_crossentropy' and no metric, so the score is the MEAN LOSS -- Keras' categorical cross-entropy
        on the softmax rows (row scaled to sum 1, clipped to [1e-7, 1 - 1e-7]).  Y: one-hot rows (n, C) as cnn.py:80-82
        builds them, or class indices (n,).  One forward, one reduction launch (mdc_crossentropy), one scalar read-back.
        nonfinite="propagate": a frame holding a NaN / +-Inf sample makes the score nan, as cnn.py:153 prints it; "raise":
        NonFiniteInputError names such frames."""
        torch = _torch()
        _nonfinite_policy(nonfinite)
        Xt = X if isinstance(X, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(X), dtype=np.float32)).to(f"cuda:{self.device_index}")
        probs = self.predict(Xt, batch_size, nonfinite=nonfinite)
        dev = probs.device
        y = Y if isinstance(Y, torch.Tensor) else torch.as_tensor(np.asarray(Y))
        if y.ndim == 2:
            if tuple(y.shape) != tuple(probs.shape):
                raise ValueError(f"one-hot targets have shape {tuple(y.shape)}, predictions {tuple(probs.shape)}")
            y = y.argmax(dim=1)
        truth = y.to(device=dev, dtype=torch.int32).contiguous()
        if truth.shape != (probs.shape[0],):
            raise ValueError(f"targets have shape {tuple(truth.shape)}, predictions {tuple(probs.shape)}")
        n, Cn = probs.shape
        if n == 0:
            return float("nan")
        loss = torch.zeros((1,), dtype=torch.float64, device=dev)
        bad = torch.zeros((1,), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            self._check(self._lib().mdc_crossentropy(probs.data_ptr(), truth.data_ptr(), n, Cn, loss.data_ptr(), bad.data_ptr(),
                                                     torch.cuda.current_stream(dev).cuda_stream))
        both = torch.cat([loss, bad.to(torch.float64)]).cpu().numpy()      # the one synchronising read
        if int(both[1]):
            raise ValueError(f"{int(both[1])} labels lie outside [0, {Cn})")
        return float(both[0] / n)

    def confusion(self, X, labels_true, batch_size: Optional[int] = None, normalize: bool = True) -> np.ndarray:
        """``conf[j,k] += 1`` over (true j, predicted k) then row-normalise, as cnn.py:199-216 does with the
        output of ``model.predict``; rows without samples stay 0."""
        conf = self.confusion_counts_device(X, labels_true, batch_size).cpu().numpy().astype(np.float64)
        if not normalize:
            return conf
        s = conf.sum(axis=1, keepdims=True)
        return np.divide(conf, s, out=np.zeros_like(conf), where=s > 0)

    def accuracy(self, X, labels_true, batch_size: Optional[int] = None) -> float:
        """cnn.py:257-259: cor / (cor + ncor) from the un-normalised confusion counts."""
        conf = self.confusion(X, labels_true, batch_size, normalize=False)
        return float(np.trace(conf) / max(conf.sum(), 1.0))

    def accuracy_by_snr(self, X, labels_true, snrs, batch_size: Optional[int] = None) -> Tuple[Dict, Dict]:
        """The per-SNR loop of cnn.py:228-259: one forward over the whole batch, then ONE launch
        (mdc_confusion_binned: an S x C x C histogram keyed by each frame's SNR bin) and one device->host copy for all
        SNR values; acc[snr] = cor / (cor + ncor) (cnn.py:257-259).  Returns (acc, conf): dicts keyed by SNR value;
        conf[snr] is the un-normalised C x C count matrix (numpy)."""
        torch = _torch()
        x = X if isinstance(X, torch.Tensor) else torch.from_numpy(
            np.ascontiguousarray(np.asarray(X), dtype=np.float32)).to(f"cuda:{self.device_index}")
        pred = self.predict_classes(x, batch_size)
        dev = pred.device
        truth = torch.as_tensor(np.asarray(labels_true) if not isinstance(labels_true, torch.Tensor) else labels_true)
        truth = truth.to(device=dev, dtype=torch.int32).contiguous()
        snr_t = torch.as_tensor(np.asarray(snrs) if not isinstance(snrs, torch.Tensor) else snrs).to(dev)
        if truth.shape != pred.shape or snr_t.shape != pred.shape:
            raise ValueError("labels_true and snrs need one entry per frame")
        Cn = self.topology.classes
        if pred.numel() == 0:
            return {}, {}
        values, bins = torch.unique(snr_t, sorted=True, return_inverse=True)      # SNR value -> bin index (plumbing)
        bins = bins.to(torch.int32).contiguous()
        S = int(values.numel())
        counts = torch.zeros((S, Cn, Cn), dtype=torch.int64, device=dev)
        bad = torch.zeros((1,), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            self._check(self._lib().mdc_confusion_binned(truth.data_ptr(), pred.data_ptr(), bins.data_ptr(), pred.numel(), Cn, S,
                                                         counts.data_ptr(), bad.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        host = torch.cat([counts.view(-1), bad]).cpu().numpy()      # the one synchronising copy
        if int(host[-1]):
            raise ValueError(f"{int(host[-1])} labels lie outside [0, {Cn})")
        c_all = host[:-1].reshape(S, Cn, Cn)
        acc, conf = {}, {}
        for i, val in enumerate(values.tolist()):
            conf[val] = c_all[i]
            acc[val] = float(np.trace(c_all[i])) / float(max(c_all[i].sum(), 1))
        return acc, conf

    @staticmethod
    def save_results(path: str, acc: Dict, tag: str = "CNN2", dr: float = 0.5) -> None:
        """The results file of cnn.py:262-264: `cPickle.dump(("CNN2", 0.5, acc), fd)` -- the tuple (model tag, dropout
        rate, {snr: accuracy}) that the reference's plotting cells read back.  Written with pickle protocol 2 (what
        Python 2's cPickle reads); keys and values are plain Python numbers."""
        import pickle
        clean = {(int(k) if float(k).is_integer() else float(k)): float(v) for k, v in acc.items()}
        with open(path, "wb") as fd:
            pickle.dump((str(tag), float(dr), clean), fd, protocol=2)

    @staticmethod
    def load_results(path: str) -> Tuple[str, float, Dict]:
        """Read back a results file: the (tag, dropout, {snr: accuracy}) tuple of save_results holds only str / float /
        int / dict / tuple, which unpickle without a single global -- so the loader REFUSES every global (class or
        function reference): a file that names one (any third party's pickle, a hostile one) raises instead of running
        code from it."""
        import pickle

        class _NoGlobals(pickle.Unpickler):
            def find_class(self, module, name):
                raise pickle.UnpicklingError(f"results files hold plain numbers and strings only; refusing {module}.{name}")

        with open(path, "rb") as fd:
            obj = _NoGlobals(fd).load()
        if not (isinstance(obj, tuple) and len(obj) == 3 and isinstance(obj[0], str) and isinstance(obj[1], (int, float))
                and isinstance(obj[2], dict)
                and all(isinstance(k, (int, float)) and isinstance(v, (int, float)) for k, v in obj[2].items())):
            raise ValueError(f"{path} is not a (tag, dropout, {{snr: accuracy}}) results file")
        tag, dr, acc = obj
        return tag, float(dr), acc

    # ------------------------------------------------------------------ FPGA arithmetic
    def predict_q612(self, X, as_float: bool = True):
        """The deployed net evaluated in the FPGA's Q6.12 integer arithmetic (mdc_forward_q612; rules of
        cnn_test_latest1.sv:642-675, 293-343).  X: float frames (n,2,128), quantised like the reference's table
        writer (`float2fix`: trunc(v*4096)), or an integer array/tensor of Q6.12 words.  Returns (dense, labels):
        the post-ReLU class sums as float (int/4096) or int32, and the first-max labels (int32)."""
        torch = _torch()
        if self.topology.kind != "deployed":
            raise ValueError("the Q6.12 datapath exists for the deployed nets only")
        as_numpy = not isinstance(X, torch.Tensor)
        t = torch.as_tensor(np.asarray(X)) if as_numpy else X
        if tuple(t.shape[1:]) != (2, 128):
            raise ValueError(f"expected input of shape (n,2,128); got {tuple(t.shape)}")
        is_q = not t.dtype.is_floating_point
        t = t.to(device=f"cuda:{self.device_index}", dtype=torch.int32 if is_q else torch.float32).contiguous()
        n, Cn = t.shape[0], self.topology.classes
        dense = torch.empty((n, Cn), dtype=torch.int32, device=t.device)
        labels = torch.empty((n,), dtype=torch.int32, device=t.device)
        self._check(self._lib().mdc_forward_q612(self._engine(), t.data_ptr() if n else None, int(is_q), n, dense.data_ptr(),
                                                 labels.data_ptr(), torch.cuda.current_stream(t.device).cuda_stream))
        out = dense.to(torch.float32) / 4096.0 if as_float else dense
        return (out.cpu().numpy(), labels.cpu().numpy()) if as_numpy else (out, labels)

    # ------------------------------------------------------------------ raw SDR bytes
    def predict_iq_u8(self, iq, scale: Optional[float] = None, batch_size: int = 0, hop: int = 128, normalize: Optional[str] = None,
                      level: float = 7.8e-3, remove_dc: bool = True, squelch_dbfs: Optional[float] = None, return_power: bool = False):
        """`predict` on raw RTL-SDR samples: iq holds unsigned bytes (I0,Q0,I1,Q1,...), each sample becomes
        (byte - 127.5) * scale (default 1/127.5).  Window i is the 128 (I,Q) pairs starting at pair i*hop of the
        capture: hop = 128 cuts it into disjoint 256-byte frames (then the byte count must be a multiple of 256),
        a smaller hop slides the classifier over a live stream (n = (pairs - 128) // hop + 1 windows).  The deployed
        nets and the VT-CNN2 family read the bytes in the forward kernels themselves (mdc_forward_iq_u8: 2*hop B of
        HBM input per window, no frame buffer); cnn.py's literal model converts on the device first
        (frames_from_iq_u8) -- the results are bit-identical either way.  Returns (probs, labels) as device tensors
        for a device tensor input, numpy arrays otherwise.

        normalize="rms": one scale PER WINDOW instead of `scale` (giving both is a ValueError) -- each window is brought to
        complex rms `level` (the level the nets were trained at), after removing each channel's mean if remove_dc
        (mdc_iq_u8_windows_norm, include/mdc.h), whatever the tuner gain and DC offset of the capture.  A device tensor runs
        chunk by chunk through mdc_iq_u8_windows_norm + mdc_forward on torch's current stream, numpy bytes through
        mdc_predict_host_iq_u8_norm; every kind of net.  squelch_dbfs (needs normalize="rms"): windows whose power
        (frontend.window_power_dbfs: 0 dBFS = a full-scale constant envelope) lies below it get label -1, their
        probabilities stay as computed.  return_power=True appends the per-window dBFS vector (float64) to the result."""
        torch = _torch()
        from .frontend import DEFAULT_SCALE, frames_from_iq_u8, window_count
        if normalize is not None:
            if normalize != "rms":
                raise ValueError(f"normalize must be None or 'rms'; got {normalize!r}")
            if scale is not None:
                raise ValueError("scale= and normalize='rms' cannot be combined: the normalised path scales each window itself")
            return self._predict_iq_u8_norm(iq, batch_size, hop, float(level), bool(remove_dc), squelch_dbfs, bool(return_power))
        if squelch_dbfs is not None or return_power:
            raise ValueError("squelch_dbfs and return_power need normalize='rms' (the plain path computes no window power)")
        scale = DEFAULT_SCALE if scale is None else float(scale)
        as_numpy = not isinstance(iq, torch.Tensor)
        if as_numpy and self.topology.kind != "cnnpy":      # host bytes: the library's streaming driver (mdc_predict_host_iq_u8)
            b = np.ascontiguousarray(np.asarray(iq, dtype=np.uint8)).reshape(-1)
            n, Cn = window_count(b.size, hop), self.topology.classes
            probs, labels = np.empty((n, Cn), np.float32), np.empty((n,), np.int32)
            self._check(self._lib().mdc_predict_host_iq_u8(self._engine(), b.ctypes.data, n, int(hop), scale, probs.ctypes.data,
                                                           labels.ctypes.data, self._host_chunk(batch_size)))
            return probs, labels
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(iq, dtype=np.uint8))) if as_numpy else iq
        if t.dtype != torch.uint8:
            raise TypeError(f"iq must be uint8, got {t.dtype}")
        t = t.to(f"cuda:{self.device_index}").contiguous().view(-1)
        n, Cn = window_count(t.numel(), hop), self.topology.classes
        if t.data_ptr() % 2:
            t = t.clone()       # a view into a larger buffer starting at an odd byte: the ABI wants whole (I,Q) pairs
        probs = torch.empty((n, Cn), dtype=torch.float32, device=t.device)
        labels = torch.empty((n,), dtype=torch.int32, device=t.device)
        if n == 0:
            return (probs.cpu().numpy(), labels.cpu().numpy()) if as_numpy else (probs, labels)
        if self.topology.kind == "cnnpy":
            x = frames_from_iq_u8(t, scale, hop=hop)
            self.forward_device(x, probs, labels, batch_size=batch_size or None)
        else:
            L, h = self._lib(), self._engine()
            chunk = max(1, min(int(batch_size) if batch_size else self.default_chunk, n))
            with torch.cuda.device(t.device):
                stream = torch.cuda.current_stream(t.device).cuda_stream
                ws, ws_bytes = self._workspace(chunk, stream)
                for s0 in range(0, n, chunk):
                    m = min(chunk, n - s0)
                    self._check(L.mdc_forward_iq_u8(h, t.data_ptr() + 2 * hop * s0, m, hop, scale,
                                                    probs.data_ptr() + s0 * Cn * 4, labels.data_ptr() + s0 * 4,
                                                    ws.data_ptr() if ws is not None else None, ws_bytes, stream))
        return (probs.cpu().numpy(), labels.cpu().numpy()) if as_numpy else (probs, labels)

    def _predict_iq_u8_norm(self, iq, batch_size, hop, level, remove_dc, squelch_dbfs, return_power):
        torch = _torch()
        from .frontend import FULL_SCALE_ENERGY, squelch_energy_threshold, window_count, window_power_dbfs
        if not (level > 0.0 and np.isfinite(level)):
            raise ValueError("level must be finite and > 0")
        flags = _cabi.IQ_REMOVE_DC if remove_dc else 0
        want_stats = squelch_dbfs is not None or return_power
        floor = squelch_energy_threshold(squelch_dbfs) if squelch_dbfs is not None else 0
        Cn = self.topology.classes
        if not isinstance(iq, torch.Tensor):      # host bytes: the library's streaming driver
            b = np.ascontiguousarray(np.asarray(iq, dtype=np.uint8)).reshape(-1)
            n = window_count(b.size, hop)
            probs, labels = np.empty((n, Cn), np.float32), np.empty((n,), np.int32)
            stats = np.empty((n,), _cabi.IQ_WINDOW_STATS) if want_stats else None
            self._check(self._lib().mdc_predict_host_iq_u8_norm(self._engine(), b.ctypes.data, n, int(hop), level, flags, probs.ctypes.data,
                                                                labels.ctypes.data, stats.ctypes.data if want_stats else None,
                                                                self._host_chunk(batch_size)))
            if squelch_dbfs is not None:
                labels[stats["energy"] < floor] = -1
            return (probs, labels, window_power_dbfs(stats)) if return_power else (probs, labels)
        if iq.dtype != torch.uint8:
            raise TypeError(f"iq must be uint8, got {iq.dtype}")
        t = iq.to(f"cuda:{self.device_index}").contiguous().view(-1)
        n = window_count(t.numel(), hop)
        if t.data_ptr() % 2:
            t = t.clone()       # a view into a larger buffer starting at an odd byte: the ABI wants whole (I,Q) pairs
        probs = torch.empty((n, Cn), dtype=torch.float32, device=t.device)
        labels = torch.empty((n,), dtype=torch.int32, device=t.device)
        stats = torch.empty((n, 4), dtype=torch.int32, device=t.device) if want_stats else None
        if n:
            L, h = self._lib(), self._engine()
            chunk = max(1, min(int(batch_size) if batch_size else self.default_chunk, n))
            with torch.cuda.device(t.device):
                stream = torch.cuda.current_stream(t.device).cuda_stream
                ws, ws_bytes = self._workspace(chunk, stream)
                x = torch.empty((chunk, 2, 128), dtype=torch.float32, device=t.device)      # one chunk of frames, reused in stream order
                for s0 in range(0, n, chunk):
                    m = min(chunk, n - s0)
                    self._check(L.mdc_iq_u8_windows_norm(t.data_ptr() + 2 * hop * s0, m, hop, level, flags, x.data_ptr(),
                                                         (stats.data_ptr() + 16 * s0) if want_stats else None, stream))
                    self._check(L.mdc_forward(h, x.data_ptr(), m, probs.data_ptr() + s0 * Cn * 4, labels.data_ptr() + s0 * 4, None,
                                              _cabi.TAP_NONE, ws.data_ptr() if ws is not None else None, ws_bytes, stream))
        if squelch_dbfs is not None:
            # (every energy is below 2^31 - 1: the int32 column holds it as it is, and a larger floor means the same as that one)
            labels.masked_fill_(stats[:, 3] < min(floor, 0x7FFFFFFF), -1)
        if return_power:
            return probs, labels, 10.0 * torch.log10(stats[:, 3].to(torch.float64) / FULL_SCALE_ENERGY)
        return probs, labels

    def predict_iq(self, iq, sample_format, scale: Optional[float] = None, batch_size: int = 0, hop: int = 128,
                   normalize: Optional[str] = None, level: float = 7.8e-3, remove_dc: bool = True, squelch_dbfs: Optional[float] = None,
                   return_power: bool = False, shift: float = 0.0, decimate: int = 1, taps=None, interpolate: int = 1):
        """predict_iq_u8 for a capture in any integer sample format: sample_format "cu8" (unsigned bytes, RTL-SDR), "ci8"
        (signed bytes: HackRF) or "ci16" (signed 16-bit little-endian: USRP sc16, SDRplay, bladeRF, Airspy); SigMF's
        "ci16_le" etc. are aliases.  iq: a numpy array or torch tensor of the format's dtype (uint8 / int8 / int16; a
        big-endian numpy int16 array is converted, any other dtype is a TypeError), flat interleaved I0,Q0,I1,Q1,... or
        shaped (..., 2).  Every sample becomes sample * scale (default 1/127.5, 1/128, 1/32768; "cu8": (byte - 127.5) * scale),
        or, with normalize="rms", each window is brought to complex rms `level` (mdc_iq_windows_norm, include/mdc.h).
        Windows, hop, batch_size, squelch_dbfs (0 dBFS = a full-scale constant envelope OF THE FORMAT) and return_power are
        predict_iq_u8's; "cu8" returns bit for bit what predict_iq_u8 returns.  A device tensor runs chunk by chunk through
        mdc_iq_windows(_norm) + mdc_forward on torch's current stream, a numpy array through mdc_predict_host_iq(_norm);
        every kind of net.

        shift / decimate / taps: a capture that is NOT yet centred on the signal or at the nets' rate (8 samples per symbol) first
        goes through the device's down-converter, frontend.ddc(iq, sample_format, shift, decimate, taps) -- shift in cycles per
        input sample is added to every frequency, taps=None is frontend.design_lowpass(decimate) --, and its int16 output is
        classified as a "ci16" capture with the same hop / normalize / level / squelch_dbfs / return_power (scale=None then means
        1/32768; hop counts OUTPUT pairs).  A numpy capture is moved to the device for this and numpy results come back.  With the
        defaults (0.0, 1, None) nothing changes.

        interpolate: a rate that no integer decimation brings to 8 samples per symbol (2.4 MS/s on 250 ksym/s wants 5/6:
        frontend.resample_ratio) goes through frontend.resample(iq, sample_format, shift, interpolate, decimate, taps) instead --
        taps=None is frontend.design_resampler of the reduced factors --; everything after it is the same.  With interpolate == 1
        the route above is taken unchanged."""
        torch = _torch()
        from . import frontend as F
        fmt = F.sample_format_id(sample_format)
        as_numpy = not isinstance(iq, torch.Tensor)
        if shift != 0.0 or decimate != 1 or taps is not None or interpolate != 1:
            if interpolate != 1:
                down = F.resample(iq, fmt, shift=shift, interpolate=interpolate, decimate=decimate, taps=taps, device=f"cuda:{self.device_index}")
            else:
                down = F.ddc(iq, fmt, shift=shift, decimate=decimate, taps=taps, device=f"cuda:{self.device_index}")
            res = self.predict_iq(down.view(-1), _cabi.IQ_CI16, scale, batch_size=batch_size, hop=hop, normalize=normalize, level=level,
                                  remove_dc=remove_dc, squelch_dbfs=squelch_dbfs, return_power=return_power)
            return tuple(r.cpu().numpy() for r in res) if as_numpy else res
        if as_numpy:
            iq = F.host_samples(iq, fmt)
        elif iq.dtype != {_cabi.IQ_CU8: torch.uint8, _cabi.IQ_CI8: torch.int8, _cabi.IQ_CI16: torch.int16}[fmt]:
            raise TypeError(f"iq must be {_cabi.IQ_SAMPLE_DTYPE[fmt].name} for sample_format {sample_format!r}, got {iq.dtype}")
        if fmt == _cabi.IQ_CU8:
            return self.predict_iq_u8(iq, scale, batch_size=batch_size, hop=hop, normalize=normalize, level=level, remove_dc=remove_dc,
                                      squelch_dbfs=squelch_dbfs, return_power=return_power)
        norm = normalize is not None
        if norm:
            if normalize != "rms":
                raise ValueError(f"normalize must be None or 'rms'; got {normalize!r}")
            if scale is not None:
                raise ValueError("scale= and normalize='rms' cannot be combined: the normalised path scales each window itself")
            gain = float(level)
            if not (gain > 0.0 and np.isfinite(gain)):
                raise ValueError("level must be finite and > 0")
        else:
            if squelch_dbfs is not None or return_power:
                raise ValueError("squelch_dbfs and return_power need normalize='rms' (the plain path computes no window power)")
            gain = F.DEFAULT_SCALES[fmt] if scale is None else float(scale)
        flags = _cabi.IQ_REMOVE_DC if remove_dc else 0
        want_stats = squelch_dbfs is not None or return_power
        floor = F.squelch_energy_threshold(squelch_dbfs, fmt) if squelch_dbfs is not None else 0
        pair, Cn = _cabi.IQ_PAIR_BYTES[fmt], self.topology.classes
        L = self._lib()
        if as_numpy:      # host samples: the library's streaming driver
            n = F.window_count(iq.nbytes, hop, pair)
            probs, labels = np.empty((n, Cn), np.float32), np.empty((n,), np.int32)
            if not norm:
                self._check(L.mdc_predict_host_iq(self._engine(), iq.ctypes.data, fmt, n, int(hop), gain, probs.ctypes.data, labels.ctypes.data,
                                                  self._host_chunk(batch_size)))
                return probs, labels
            stats = np.empty((n,), _cabi.IQ_WINDOW_STATS64) if want_stats else None
            self._check(L.mdc_predict_host_iq_norm(self._engine(), iq.ctypes.data, fmt, n, int(hop), gain, flags, probs.ctypes.data,
                                                   labels.ctypes.data, stats.ctypes.data if want_stats else None, self._host_chunk(batch_size)))
            if squelch_dbfs is not None:
                labels[stats["energy"] < np.uint64(floor)] = -1
            return (probs, labels, F.window_power_dbfs(stats, fmt)) if return_power else (probs, labels)
        t = iq.to(f"cuda:{self.device_index}").contiguous().view(-1)
        n = F.window_count(t.numel() * t.element_size(), hop, pair)
        if t.data_ptr() % pair:
            t = t.clone()       # a view into a larger buffer starting inside a pair: the ABI wants whole (I,Q) pairs
        probs = torch.empty((n, Cn), dtype=torch.float32, device=t.device)
        labels = torch.empty((n,), dtype=torch.int32, device=t.device)
        stats = torch.empty((n, 4), dtype=torch.int64, device=t.device) if want_stats else None
        if n:
            h = self._engine()
            chunk = max(1, min(int(batch_size) if batch_size else self.default_chunk, n))
            with torch.cuda.device(t.device):
                stream = torch.cuda.current_stream(t.device).cuda_stream
                ws, ws_bytes = self._workspace(chunk, stream)
                x = torch.empty((chunk, 2, 128), dtype=torch.float32, device=t.device)      # one chunk of frames, reused in stream order
                for s0 in range(0, n, chunk):
                    m = min(chunk, n - s0)
                    src = t.data_ptr() + pair * hop * s0
                    if norm:
                        self._check(L.mdc_iq_windows_norm(src, fmt, m, hop, gain, flags, x.data_ptr(),
                                                          (stats.data_ptr() + 32 * s0) if want_stats else None, stream))
                    else:
                        self._check(L.mdc_iq_windows(src, fmt, m, hop, gain, x.data_ptr(), stream))
                    self._check(L.mdc_forward(h, x.data_ptr(), m, probs.data_ptr() + s0 * Cn * 4, labels.data_ptr() + s0 * 4, None,
                                              _cabi.TAP_NONE, ws.data_ptr() if ws is not None else None, ws_bytes, stream))
        if squelch_dbfs is not None:
            labels.masked_fill_(stats[:, 3] < floor, -1)      # (64-bit energies: every E and every floor is below 2^47)
        if return_power:
            return probs, labels, 10.0 * torch.log10(stats[:, 3].to(torch.float64) / F.full_scale_energy(fmt))
        return probs, labels

    def scan_iq(self, iq, sample_format, nfft: int = 1024, avg: int = 8, threshold_db: float = 6.0, hop: int = 128, level: float = 7.8e-3,
                squelch_dbfs: Optional[float] = None, refine: bool = False, min_line_db: float = 8.0, bursts: bool = False, hold: float = 0.98,
                burst_threshold_db: float = 3.0, min_rows: int = 1, merge_rows: int = 1, **find_kw):
        """A wideband capture in, "what is transmitting where, and what modulation" out.  The capture's power spectrogram
        (frontend.spectrogram: nfft bins, Hann window, segments nfft // 2 apart, `avg` of them per row, on the device) is averaged
        over its rows into one spectrum; frontend.find_emitters(spectrum, threshold_db, window=the Hann window, **find_kw) lists
        the emitters; each one is brought to 0 Hz and to the nets' rate by frontend.channel_plan's (shift, L, D) -- through
        frontend.ddc when L == 1, else frontend.resample, with frontend.plan_taps(L, D) as the filter --, cut into windows `hop` output pairs apart
        (hop == 128: the stream is trimmed to whole frames) and classified with predict_iq(..., "ci16", normalize="rms", level=,
        squelch_dbfs=, return_power=True).  Returns one dict per emitter, in order of centre: centre, bandwidth (cycles per input
        sample), power_dbfs, snr_db, shift, interpolate, decimate, probs, labels, window_dbfs (predict_iq's three results: device
        tensors, or numpy arrays for a numpy capture) and label, the most frequent label among the windows the squelch let through
        (the smallest on a tie; -1 if there are none).

        refine=True replaces the plan's two guesses -- a symbol rate from the thresholded width, a carrier from the centroid -- by
        the emitter's spectral lines.  Per emitter: (1) isolate it at about four times its width, D0 = clamp(floor(1 / (4
        bandwidth)), 1, 256), iso = frontend.ddc(capture, shift=-centre, decimate=D0, taps=frontend.plan_taps(1, D0)); b =
        bandwidth D0 is its width there.  (2) frontend.estimate_symbol_rate(iso, "ci16", lo=b / 2.5, hi=min(0.45, 1.25 b),
        min_line_db=): a linear modulation's symbol rate is b / (1 + beta), beta in 0..1, and a thresholded width may be 25 % off;
        the band also keeps the line's harmonics out.  symbol_rate = rate / D0 (None without a line).  (3)
        frontend.estimate_carrier_offset(iso, "ci16", max_offset=b / 8, min_line_db=) (at most 0.12: an emitter filling the whole
        band); carrier_offset = offset / D0, and shift = -(centre + carrier_offset), folded into [-0.5, 0.5].  (4) (L, D) = frontend.resample_ratio(1.0, symbol_rate, 8) when the symbol line was found and
        a ratio within its 1 % exists, else channel_plan's.  (5) The ORIGINAL capture is resampled with that shift and ratio and
        plan_taps(L, D), and classified as above.  The record gains symbol_rate (cycles per input sample, or None),
        symbol_line_db, carrier_offset, carrier_order (2, 4, or 0: no line -- 8PSK, analogue and frequency-shift signals show
        none -- and the centroid stands) and carrier_line_db; centre stays the centroid.  refine=False is the plan alone, and its
        record has none of the five.

        bursts=True is the scan for INTERMITTENT emitters -- push-to-talk, telemetry bursts, packet traffic --, which the mean over
        the rows dilutes (on 3 % of the time: by 15 dB) until they are missed or found in fragments.  The spectrogram is then looked
        at along time per bin: Q = frontend.spectrum_quantiles(spec, (0.5, hold)), one call on the device.  The emitters are
        find_emitters(Q[1], threshold_db, ...): the spectrum each bin reaches in its top 1 - hold of the rows, whose own median bin
        is find_emitters' floor, so that the noise's high quantile cancels.  The noise per bin is the median over the bins of
        Q[0], the median over time, which bursts do not lift.  Per emitter, (first, count) = frontend.emitter_bins(e, nfft), band =
        frontend.band_power(spec, first, count), and frontend.find_bursts(band, count * noise, burst_threshold_db, min_rows,
        merge_rows) gives the rows it was on.  The record gains bursts, a list of half-open intervals of INPUT pairs
        (frontend.burst_pairs), and duty, on-rows / rows.  Plan, refine, tuning, resampling and predict_iq run on the whole
        capture as without bursts; then every window whose frontend.window_support (the input pairs its 128 outputs read through
        the filter) is not wholly inside one burst gets label -1, as the squelch does, and label is the majority among the
        windows still open; probs and window_dbfs are untouched.  A spectrogram's rows drop trailing segments that do not fill a
        row (and a window's support is wider than the window): the last windows of a capture can therefore be gated even for an
        emitter that never pauses.  An emitter must revisit its bins in at least 1 - hold of the rows to be seen.  bursts=False
        (the default) is the mean spectrum, and its record has neither key."""
        torch = _torch()
        from . import frontend as F
        fmt = F.sample_format_id(sample_format)
        as_numpy = not isinstance(iq, torch.Tensor)
        dev = F._device_samples(iq, fmt, f"cuda:{self.device_index}")
        window = F.design_window(nfft)
        spec = F.spectrogram(dev, fmt, nfft=nfft, avg=avg)
        if spec.shape[0] == 0:
            raise ValueError(f"the capture is too short for one row of {avg} segments of {nfft} pairs")
        if bursts:
            quant = F.spectrum_quantiles(spec, (0.5, float(hold))).to(torch.float64).cpu().numpy()
            psd, noise = quant[1], float(np.median(quant[0]))
        else:
            psd = spec.to(torch.float64).mean(0).cpu().numpy()
        out = []
        for e in F.find_emitters(psd, threshold_db=threshold_db, window=window, **find_kw):
            shift, L, D, _ = F.channel_plan(e.centre, e.bandwidth)
            extra = {}
            if refine:
                D0 = min(max(int(1.0 / (4.0 * e.bandwidth)), 1), 256)
                iso = F.ddc(dev, fmt, shift=-e.centre, decimate=D0, taps=F.plan_taps(1, D0)).reshape(-1)
                b = e.bandwidth * D0
                rate, rate_db = F.estimate_symbol_rate(iso, _cabi.IQ_CI16, lo=b / 2.5, hi=min(0.45, 1.25 * b), min_line_db=min_line_db)
                offset, order, offset_db = F.estimate_carrier_offset(iso, _cabi.IQ_CI16, max_offset=min(b / 8.0, 0.12), min_line_db=min_line_db)
                shift = -(e.centre + offset / D0)
                if abs(shift) > 0.5:      # an emitter at the band's edge: the same frequency, one turn on
                    shift -= round(shift)
                if rate is not None:
                    try:
                        L, D, _ = F.resample_ratio(1.0, rate / D0, 8)
                    except ValueError:      # nothing within 1 %: the plan's ratio stands
                        pass
                extra = dict(symbol_rate=None if rate is None else rate / D0, symbol_line_db=rate_db, carrier_offset=offset / D0, carrier_order=order,
                             carrier_line_db=offset_db)
            taps = F.plan_taps(L, D)
            if L == 1:
                down = F.ddc(dev, fmt, shift=shift, decimate=D, taps=taps)
            else:
                down = F.resample(dev, fmt, shift=shift, interpolate=L, decimate=D, taps=taps)
            if hop == 128:
                down = down[:down.shape[0] // 128 * 128]
            probs, labels, dbfs = self.predict_iq(down.reshape(-1), _cabi.IQ_CI16, hop=hop, normalize="rms", level=level, squelch_dbfs=squelch_dbfs,
                                                  return_power=True)
            if bursts:
                first_bin, count = F.emitter_bins(e, nfft)
                rows_on = F.find_bursts(F.band_power(spec, first_bin, count).cpu(), count * noise, burst_threshold_db, min_rows, merge_rows)
                on = [F.burst_pairs(a, z, nfft, nfft // 2, avg) for a, z in rows_on]
                extra.update(bursts=on, duty=sum(z - a for a, z in rows_on) / spec.shape[0])
                lo, hi = F._window_supports(np.arange(labels.shape[0]), hop, taps.size, L, D)
                inside = np.zeros(labels.shape[0], bool)
                for a, z in on:
                    inside |= (lo >= a) & (hi < z)
                labels.masked_fill_(torch.from_numpy(~inside).to(labels.device), -1)
            open_ = labels[labels >= 0]
            label = int(torch.bincount(open_).argmax()) if open_.numel() else -1
            if as_numpy:
                probs, labels, dbfs = probs.cpu().numpy(), labels.cpu().numpy(), dbfs.cpu().numpy()
            out.append(dict(centre=e.centre, bandwidth=e.bandwidth, power_dbfs=e.power_dbfs, snr_db=e.snr_db, shift=shift, interpolate=L, decimate=D,
                            labels=labels, probs=probs, window_dbfs=dbfs, label=label, **extra))
        return out

    def detect_iq(self, iq, sample_format, nfft: int = 1024, avg: int = 8, threshold_db: float = 6.0, floor: str = "flat", reach_rows: int = 2,
                  reach_bins: int = 3, min_rows: int = 3, min_bins: int = 3, hop: int = 128, level: float = 7.8e-3,
                  squelch_dbfs: Optional[float] = None, dc_guard: int = 1, batched: bool = False, refine: bool = False, min_line_db: float = 8.0,
                  line_nfft: int = 1024, line_avg: int = 8):
        """A wideband capture in, "what transmitted when, where, and what modulation" out: the scan in two dimensions, for
        frequency hoppers, emitters that share bins at different times and single packets, which scan_iq's one-dimensional
        searches miss or mangle.  The capture's spectrogram (frontend.spectrogram, as scan_iq builds it: nfft bins, segments nfft //
        2 apart, `avg` per row) is thresholded per cell at frontend.detection_threshold(spec, threshold_db, dc_guard, floor) and
        frontend.find_detections(spec, thresh, reach_rows, reach_bins, min_rows, min_bins, avg=avg) joins the on-cells into boxes
        in time and frequency, all on the device.  Per detection, frontend.channel_plan(centre, bandwidth) and frontend.plan_taps
        give (shift, L, D) and the filter, and ONLY the pairs [first_pair, stop_pair) of the capture go through frontend.ddc (L ==
        1) or frontend.resample; the result is cut into windows `hop` output pairs apart (hop == 128: trimmed to whole frames)
        and classified with predict_iq(..., "ci16", normalize="rms", level=, squelch_dbfs=, return_power=True).  Returns one dict
        per detection, ordered by (first_pair, centre): the Detection's fields (first_row, stop_row, first_bin, stop_bin, cells,
        centre, bandwidth, peak_db, snr_db, first_pair, stop_pair) plus shift, interpolate, decimate, probs, labels, window_dbfs
        (device tensors, or numpy arrays for a numpy capture), windows, their number, and label, the most frequent label among the
        windows the squelch let through (the smallest on a tie; -1 if there are none).  A detection whose pairs are too few for
        one window gives windows = 0, label = -1 and empty results.  The default dc_guard of 1 switches bins -1, 0, +1 off, a gap
        of three that reach_bins = 3 does not bridge: an emitter ON bin 0 comes out as two boxes, one each side of the guard.  A
        capture without a DC spike takes dc_guard=0 (only bin 0 off) and gets it as one.
        batched=True gives the same records, key for key and bit for bit, without the loop over detections: one
        frontend.extract launch tunes, filters and resamples every detection's pairs into one block of whole frames, one
        predict_iq classifies the block, frontend.segment_votes takes every detection's vote on the device, and the labels come to
        the host in one transfer; probs, labels and window_dbfs are then slices of the block's results.  It needs hop == 128 (with
        another hop windows would straddle detections: ValueError).
        refine=True replaces the plan's two guesses per detection -- a symbol rate from the box's width, a carrier from its
        centroid -- by the detection's spectral lines, scan_iq(refine=True)'s recipe on the detection's own pairs: D0 = clamp(floor(1
        / (4 bandwidth)), 1, 256); iso = the pairs [first_pair, stop_pair) through frontend.ddc(shift=-centre, decimate=D0,
        taps=frontend.plan_taps(1, D0)); b = bandwidth D0.  frontend.line_spectra(iso, "ci16", orders (0, 2, 4), nfft=line_nfft,
        avg=line_avg) gives the three mean spectra, frontend.find_lines searches the envelope's in [b / 2.5, min(0.45, 1.25 b)] and,
        with m = min(b / 8, 0.12), the square's in |f| <= 2 m and the fourth power's in |f| <= 4 m.  The symbol line counts from
        min_line_db on (frontend.estimate_symbol_rate's rule); the carrier is order 2's line if it reaches min_line_db, else order
        4's, else none (frontend.estimate_carrier_offset's rule).  shift = -(centre + offset / D0), folded into [-0.5, 0.5]; (L, D) =
        frontend.resample_ratio(1.0, rate / D0, 8) when the symbol line was found and a ratio within its 1 % exists, else the plan's.
        The record gains symbol_rate (cycles per input sample, or None), symbol_line_db, carrier_offset, carrier_order (2, 4, or 0)
        and carrier_line_db; centre stays the centroid.  A detection too short for one row of line_avg segments of line_nfft
        isolated pairs, or whose symbol band holds no bin at line_nfft, keeps the plan: symbol_rate None, symbol_line_db -inf,
        carrier_offset 0.0, carrier_order 0, carrier_line_db -inf.  The loop does ddc, line_spectra (one job) and find_lines (three
        bands) per detection; batched=True does ONE frontend.extract(..., whole_frames=False) for all isolations, ONE line_spectra
        over the block, ONE find_lines whose 3 K records come to the host in one transfer, and then the extraction above with the
        refined shifts and ratios: the same spectra from the same entries, so both forms agree bit for bit.  refine=False is the
        plan alone, and its record has none of the five keys."""
        torch = _torch()
        from . import frontend as F
        fmt = F.sample_format_id(sample_format)
        if batched and hop != 128:
            raise ValueError(f"batched=True needs hop == 128 (got {hop}): windows at another hop would straddle two detections")
        as_numpy = not isinstance(iq, torch.Tensor)
        dev = F._device_samples(iq, fmt, f"cuda:{self.device_index}")
        spec = F.spectrogram(dev, fmt, nfft=nfft, avg=avg)
        if spec.shape[0] == 0:
            raise ValueError(f"the capture is too short for one row of {avg} segments of {nfft} pairs")
        thresh = F.detection_threshold(spec, threshold_db, dc_guard, floor)
        if batched:
            found = F.find_detections(spec, thresh, reach_rows, reach_bins, min_rows, min_bins, avg=avg)
            if not refine:
                return self._classify_detections(dev, fmt, found, level, squelch_dbfs, as_numpy)
            plans, extras = self._refine_detections(dev, fmt, found, min_line_db, line_nfft, line_avg)
            return self._classify_detections(dev, fmt, found, level, squelch_dbfs, as_numpy, plans, extras)
        per_pair = _cabi.IQ_PAIR_BYTES[fmt] // dev.element_size()      # elements of `dev` per (I,Q) pair
        Cn = self.topology.classes
        out = []
        for d in F.find_detections(spec, thresh, reach_rows, reach_bins, min_rows, min_bins, avg=avg):
            shift, L, D, _ = F.channel_plan(d.centre, d.bandwidth)
            part = dev[d.first_pair * per_pair:d.stop_pair * per_pair]
            extra = {}
            if refine:
                D0, bands = self._line_bands(d.bandwidth, line_nfft)
                lines = None
                if bands is not None:
                    iso = F.ddc(part, fmt, shift=-d.centre, decimate=D0, taps=F.plan_taps(1, D0))
                    means, rows = F.line_spectra(iso.reshape(-1), _cabi.IQ_CI16, [(0, iso.shape[0])], orders=(0, 2, 4), nfft=line_nfft, avg=line_avg)
                    if rows[0] > 0:
                        lines = F.find_lines(means[0], bands)
                (shift, L, D), extra = self._refined_plan(d.centre, D0, (shift, L, D), lines, min_line_db)
            taps = F.plan_taps(L, D)
            if L == 1:
                n_out = F.ddc_out_count(d.stop_pair - d.first_pair, taps.size, D)
            else:
                n_out = F.resample_out_count(d.stop_pair - d.first_pair, taps.size, L, D)
            if n_out < 128:
                probs = torch.empty((0, Cn), dtype=torch.float32, device=dev.device)
                labels = torch.empty((0,), dtype=torch.int32, device=dev.device)
                dbfs = torch.empty((0,), dtype=torch.float64, device=dev.device)
            else:
                if L == 1:
                    down = F.ddc(part, fmt, shift=shift, decimate=D, taps=taps)
                else:
                    down = F.resample(part, fmt, shift=shift, interpolate=L, decimate=D, taps=taps)
                if hop == 128:
                    down = down[:down.shape[0] // 128 * 128]
                probs, labels, dbfs = self.predict_iq(down.reshape(-1), _cabi.IQ_CI16, hop=hop, normalize="rms", level=level,
                                                      squelch_dbfs=squelch_dbfs, return_power=True)
            open_ = labels[labels >= 0]
            label = int(torch.bincount(open_).argmax()) if open_.numel() else -1
            windows = int(labels.shape[0])
            if as_numpy:
                probs, labels, dbfs = probs.cpu().numpy(), labels.cpu().numpy(), dbfs.cpu().numpy()
            out.append(dict(d._asdict(), shift=shift, interpolate=L, decimate=D, probs=probs, labels=labels, window_dbfs=dbfs, windows=windows,
                            label=label, **extra))
        return out

    @staticmethod
    def _line_bands(bandwidth, line_nfft):
        """detect_iq(refine=True): (D0, bands) of a detection of that bandwidth -- the isolating decimation and the three bands of
        frontend.find_lines (envelope, square, fourth power) at its isolated rate; bands is None when the envelope's band holds
        no bin of line_nfft"""
        D0 = min(max(int(1.0 / (4.0 * bandwidth)), 1), 256)
        b = bandwidth * D0
        lo, hi = b / 2.5, min(0.45, 1.25 * b)
        f = np.fft.fftfreq(int(line_nfft))
        if not np.any((f >= lo) & (f <= hi)):
            return D0, None
        m = min(b / 8.0, 0.12)
        return D0, [(lo, hi, False), (0.0, 2.0 * m, True), (0.0, 4.0 * m, True)]

    @staticmethod
    def _refined_plan(centre, D0, plan, lines, min_line_db):
        """detect_iq(refine=True): ((shift, L, D), the record's five extra keys) from find_lines' three results at orders 0, 2, 4
        of the detection isolated at decimation D0 (lines None: no spectrum, the plan stands) -- the decisions of
        frontend.estimate_symbol_rate and frontend.estimate_carrier_offset, and scan_iq(refine=True)'s use of them"""
        from . import frontend as F
        if lines is None:
            return plan, dict(symbol_rate=None, symbol_line_db=float("-inf"), carrier_offset=0.0, carrier_order=0, carrier_line_db=float("-inf"))
        shift, L, D = plan
        (rate, rate_db), (f2, db2), (f4, db4) = lines
        if rate_db < float(min_line_db):
            rate = None
        if db2 >= float(min_line_db):
            offset, order, offset_db = f2 / 2, 2, db2
        elif db4 >= float(min_line_db):
            offset, order, offset_db = f4 / 4, 4, db4
        else:
            offset, order, offset_db = 0.0, 0, max(db2, db4)
        shift = -(centre + offset / D0)
        if abs(shift) > 0.5:      # a detection at the band's edge: the same frequency, one turn on
            shift -= round(shift)
        if rate is not None:
            try:
                L, D, _ = F.resample_ratio(1.0, rate / D0, 8)
            except ValueError:      # nothing within 1 %: the plan's ratio stands
                pass
        return (shift, L, D), dict(symbol_rate=None if rate is None else rate / D0, symbol_line_db=rate_db, carrier_offset=offset / D0,
                                   carrier_order=order, carrier_line_db=offset_db)

    def _refine_detections(self, dev, fmt, found, min_line_db, line_nfft, line_avg):
        """detect_iq(batched=True, refine=True) before the extraction: (plans, extras) of all detections from one frontend.extract
        of their isolations, one frontend.line_spectra over that block and one frontend.find_lines"""
        from . import frontend as F
        plans = [p[:3] for p in F.channel_plans([(d.centre, d.bandwidth) for d in found])]
        if not found:
            return plans, []
        geo = [self._line_bands(d.bandwidth, line_nfft) for d in found]
        taps = {}
        for D0, _ in geo:
            if D0 not in taps:
                taps[D0] = F.plan_taps(1, D0)
        block, offsets = F.extract(dev, fmt, [(d.first_pair, d.stop_pair, -d.centre, 1, D0, taps[D0]) for d, (D0, _) in zip(found, geo)],
                                   whole_frames=False)
        means, rows = F.line_spectra(block.reshape(-1), _cabi.IQ_CI16, offsets, orders=(0, 2, 4), nfft=line_nfft, avg=line_avg)
        live = [k for k, (_, bands) in enumerate(geo) if bands is not None and rows[k] > 0]
        lines = {}
        if live:
            at = _torch().as_tensor(live, dtype=_torch().int64, device=means.device)
            got = F.find_lines(means[at].reshape(-1, means.shape[2]), [band for k in live for band in geo[k][1]])
            lines = {k: got[3 * i:3 * i + 3] for i, k in enumerate(live)}
        out = [self._refined_plan(d.centre, D0, plan, lines.get(k), min_line_db) for k, (d, (D0, _), plan) in enumerate(zip(found, geo, plans))]
        return [p for p, _ in out], [e for _, e in out]

    def _classify_detections(self, dev, fmt, found, level, squelch_dbfs, as_numpy, plans=None, extras=None):
        """detect_iq(batched=True) behind the search: the records of `found` (frontend.find_detections) on the device capture dev;
        plans: (shift, L, D) per detection, None = frontend.channel_plans'; extras: per detection, further keys of its record"""
        torch = _torch()
        from . import frontend as F
        if not found:
            return []
        Cn = self.topology.classes
        if plans is None:
            plans = [p[:3] for p in F.channel_plans([(d.centre, d.bandwidth) for d in found])]
        taps = {}
        for _, L, D in plans:
            if (L, D) not in taps:
                taps[L, D] = F.plan_taps(L, D)
        block, offsets = F.extract(dev, fmt, [(d.first_pair, d.stop_pair, shift, L, D, taps[L, D]) for d, (shift, L, D) in zip(found, plans)],
                                   whole_frames=True)
        first = (offsets // 128).tolist()      # in windows
        if block.shape[0]:
            probs, labels, dbfs = self.predict_iq(block.reshape(-1), _cabi.IQ_CI16, normalize="rms", level=level, squelch_dbfs=squelch_dbfs,
                                                  return_power=True)
        else:
            probs = torch.empty((0, Cn), dtype=torch.float32, device=dev.device)
            labels = torch.empty((0,), dtype=torch.int32, device=dev.device)
            dbfs = torch.empty((0,), dtype=torch.float64, device=dev.device)
        label = F.segment_votes(labels, offsets // 128, Cn).cpu().tolist()      # the one transfer of the K labels
        if as_numpy:
            probs, labels, dbfs = probs.cpu().numpy(), labels.cpu().numpy(), dbfs.cpu().numpy()
        out = []
        for k, (d, (shift, L, D)) in enumerate(zip(found, plans)):
            a, z = first[k], first[k + 1]
            out.append(dict(d._asdict(), shift=shift, interpolate=L, decimate=D, probs=probs[a:z], labels=labels[a:z], window_dbfs=dbfs[a:z],
                            windows=z - a, label=label[k], **(extras[k] if extras else {})))
        return out

    def predict_channels(self, iq, sample_format, channels: int, decimate: Optional[int] = None, taps=None, tap_shift: Optional[int] = None,
                         hop: int = 128, level: float = 7.8e-3, squelch_dbfs: Optional[float] = None, batch_size: int = 0):
        """A band with a channel raster in, "what is on every channel" out.  The capture is split into M = channels evenly spaced
        channels in one pass (frontend.channelize(iq, sample_format, channels, decimate, taps, tap_shift, whole_frames=True):
        decimate=None is M / 2, taps=None frontend.design_channelizer(M)), and every channel's stream is cut into windows `hop`
        output pairs apart and classified with predict_iq(..., "ci16", normalize="rms", level=, squelch_dbfs=, return_power=True).
        With hop == 128 that is ONE predict_iq call over the flat (M * n_out) block: the rows are whole frames, so no window
        straddles two channels; other hops go channel by channel.  Returns probs (M, W, C), labels (M, W), window_dbfs (M, W) and
        label (M,), int64: per channel the most frequent label among the windows the squelch let through (the smallest on a tie;
        -1 if there are none) -- scan_iq's rule.  Row k is the channel centred at frontend.channel_freqs(M)[k].  Device tensors
        for a device capture, numpy arrays for a numpy capture."""
        torch = _torch()
        from . import frontend as F
        fmt = F.sample_format_id(sample_format)
        as_numpy = not isinstance(iq, torch.Tensor)
        down = F.channelize(iq, fmt, channels, decimate=decimate, taps=taps, tap_shift=tap_shift, whole_frames=True,
                            device=f"cuda:{self.device_index}")
        M, n_out = down.shape[0], down.shape[1]
        kw = dict(batch_size=batch_size, hop=hop, normalize="rms", level=level, squelch_dbfs=squelch_dbfs, return_power=True)
        if hop == 128:
            probs, labels, dbfs = self.predict_iq(down.view(-1), _cabi.IQ_CI16, **kw)
            W = n_out // 128
            probs, labels, dbfs = probs.view(M, W, self.topology.classes), labels.view(M, W), dbfs.view(M, W)
        else:
            per = [self.predict_iq(down[k].reshape(-1), _cabi.IQ_CI16, **kw) for k in range(M)]
            probs, labels, dbfs = (torch.stack([p[i] for p in per]) for i in range(3))
        classes = torch.arange(self.topology.classes, dtype=labels.dtype, device=labels.device)
        counts = (labels[:, :, None] == classes).sum(1)      # (M, C): squelched windows (-1) count for no class
        label = torch.where(counts.sum(1) > 0, counts.argmax(1), torch.full((M,), -1, dtype=torch.int64, device=labels.device))
        if as_numpy:
            return probs.cpu().numpy(), labels.cpu().numpy(), dbfs.cpu().numpy(), label.cpu().numpy()
        return probs, labels, dbfs, label

    # ------------------------------------------------------------------ measurement hooks
    def set_profiling(self, on: bool) -> None:
        self._check(self._lib().mdc_set_profiling(self._engine(), int(on)))
        if on:
            self._check(self._lib().mdc_profile_reset(self._engine()))

    def read_profile(self) -> Dict[str, Tuple[float, int]]:
        L, h = self._lib(), self._engine()
        out = {}
        for i in range(L.mdc_profile_slots(h)):
            ms, cnt = C.c_double(), C.c_int64()
            self._check(L.mdc_profile_read(h, i, C.byref(ms), C.byref(cnt)))
            out[L.mdc_profile_name(h, i).decode()] = (ms.value, cnt.value)
        return out


# ----------------------------------------------------------------------------------------------------------------------
# CNN.ipynb cell 17 spelled as the notebook spells it:
#     model2 = Model(inputs = model.inputs, outputs = model.layers[4].output)   # dense + ReLU, no softmax
#     model2.compile(loss='categorical_crossentropy', optimizer='adam'); model2.predict(np.array([X_test[i],]))
# A sub-model is a VIEW of its parent: the same device weights, one forward with the layer's tap (MDC_TAP_*), the result in
# the shape Keras gives that layer's output.  Layers whose output the kernels never materialise (the input reshapes and
# paddings, VT-CNN2's first convolution -- conv1 feeds conv2 from registers) have no tap and say so.
# ----------------------------------------------------------------------------------------------------------------------
class ModelInputs:
    def __init__(self, model: VTCNN2):
        self.model = model

    def __repr__(self):
        return "[<input (None, 2, 128) float32>]"


class LayerOutput:
    def __init__(self, layer: "Layer"):
        self.layer = layer

    @property
    def shape(self):
        return self.layer.output_shape

    def __repr__(self):
        return f"<output of {self.layer!r} {self.layer.output_shape}>"


class Layer:
    """One entry of `model.layers`: what the reference prints, reads weights from and taps."""

    def __init__(self, model: VTCNN2, index: int, class_name: str, name: str, shape: Tuple[int, ...], params: int):
        self.model, self.index, self.class_name, self.name = model, index, class_name, name
        self.output_shape = (None,) + tuple(shape)
        self._params = params

    def __repr__(self):
        return f"<{self.class_name} {self.name}>"

    def count_params(self) -> int:
        return self._params

    def get_weights(self) -> List[np.ndarray]:
        """[kernel, bias] of a Conv2D / Dense in the layout Keras holds them, [] for the others (`layer.get_weights()`)."""
        if self._params == 0:
            return []
        rows = self.model.topology.keras_layers()
        k = sum(1 for _c, _s, p in rows[:self.index] if p)
        kernel, bias = self.model.get_weights()[k]
        return [kernel, bias]

    @property
    def output(self) -> LayerOutput:
        return LayerOutput(self)

    @property
    def tap(self) -> Optional[str]:
        """The MDC_TAP_* name that yields this layer's output; None = the model's own output (softmax rows)."""
        kind, i = self.model.topology.kind, self.index
        table = {"deployed": {2: "conv", 3: "flat", 4: "dense", 5: None, 6: None},
                 "cnnpy": {2: "conv", 3: "flat", 4: "hidden", 5: "dense", 6: None, 7: None},
                 # Dropout is the identity at inference: its output is its input's
                 "vtcnn2": {5: "conv", 6: "conv", 7: "flat", 8: "hidden", 9: "hidden", 10: "dense", 11: None, 12: None}}[kind]
        if i not in table:
            raise ValueError(f"{self!r}: this layer's output is never materialised by the kernels (input reshapes / paddings; "
                             "VT-CNN2's conv1 feeds conv2 from registers) -- no tap")
        return table[i]


class SubModel:
    """`Model(inputs=model.inputs, outputs=model.layers[i].output)`: predict() = one forward of the parent with that tap."""

    def __init__(self, parent: VTCNN2, layer: Layer):
        self.parent, self.layer, self._tap = parent, layer, layer.tap      # (raises here for a layer without a tap)

    def compile(self, *_a, **_k) -> None:
        """The notebook compiles its sub-models before predicting; nothing to prepare here."""

    @property
    def output_shape(self):
        return self.layer.output_shape

    def predict(self, X, batch_size: Optional[int] = None, verbose: int = 0):
        out = self.parent.predict(X, batch_size=batch_size, tap=self._tap)
        return out.reshape((out.shape[0],) + tuple(self.layer.output_shape[1:]))


def Model(inputs=None, outputs=None) -> SubModel:
    """keras.models.Model(inputs=model.inputs, outputs=model.layers[i].output) for a layer of a VTCNN2 (CNN.ipynb cell 17)."""
    if not isinstance(outputs, LayerOutput):
        raise TypeError("outputs must be `model.layers[i].output` of a VTCNN2")
    parent = outputs.layer.model
    if inputs is not None and not (isinstance(inputs, ModelInputs) and inputs.model is parent):
        raise ValueError("inputs must be the same model's `model.inputs`")
    return SubModel(parent, outputs.layer)
