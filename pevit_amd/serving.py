"""Serving: an engine context that can ONLY infer (``pevit_infer_create``, include/pevit_hip.h), a frozen tower loaded once, and
any number of adapter checkpoints (``adapter_io``) resident next to it and swapped in by pointer.

The context's arena holds no transposed weight copy and its workspace no slot that only a backward pass touches; what it computes
is ``HipEngine.predict`` / ``encode_image`` / ``zeroshot`` bit for bit -- the same kernels on the same operands.  Train with
``HipEngine`` (or the fine-tune harness), ``save_adapter``, then::

    eng = InferenceEngine(arch, "kadaptation", max_classes=100, max_batch=128)
    eng.load_backbone(clip_state_dict)
    eng.add_adapter("cifar100", "adapter_cifar100_kadaptation.pt")
    eng.use("cifar100")
    logits = eng.predict(images)            # any number of images, in chunks of max_batch
"""
from __future__ import annotations

import os

import torch

from . import _lib, adapter_io
from ._context import EngineContext
from .engine_input import InputMixin
from .synth import VitArch


class InferenceEngine(EngineContext, InputMixin):
    """One inference-only context.  All of its state -- also what ``InputMixin`` rebinds -- is declared in ``__init__``."""

    def __init__(self, arch: VitArch, method: str, max_classes: int, max_batch: int, lora_rank: int = 4,
                 device: str | torch.device = "cuda:0", weight_format: str = "bf16"):
        super().__init__(device)
        self.arch, self.method, self.max_classes, self.lora_rank, self.max_batch = arch, method, int(max_classes), lora_rank, int(max_batch)
        if weight_format not in _lib.WEIGHT_FORMATS:
            raise ValueError(f"weight_format {weight_format!r}: expected one of {sorted(_lib.WEIGHT_FORMATS)}")
        self.weight_format = weight_format
        dims = _lib.PevitDims(arch.width, arch.layers, arch.patch, arch.resolution, arch.embed_dim,
                              _lib.METHOD_IDS[method], lora_rank, self.max_classes, _lib.WEIGHT_FORMATS[weight_format])
        self._create("pevit_infer_create", dims, self.max_batch)
        self.n_tower = self.lib.pevit_num_tower_params(self._ctx)
        self._adapters = {}              # name -> {"params", "running_mean", "running_var", "phm_rule" (device), "num_classes", "meta"}
        self._current = None             # the name ``use`` selected
        self._backbone_sha256 = None     # adapter_io.backbone_fingerprint of the tower load_backbone read
        # ---- engine_input.py
        self._input_norm = None          # (mean, std) once set_input_normalization has run: uint8 batches are taken from then on
        self._input_resize, self._resize_center_crop = False, True       # set_input_resize(on, center_crop)
        self._resize_buf, self._resize_cache = None, {}  # resize_u8: its staging (on first use), (h, w, crop) -> device tables

    @property
    def arena_bytes(self) -> int:
        return self.arena.numel()

    @property
    def workspace_bytes(self) -> int:
        return self.workspace.numel()

    # ------------------------------------------------------------------ the frozen tower
    def load_backbone(self, sd, prefix: str = "visual."):
        """Frozen tower from an OpenAI-layout state dict (any float dtype, any device): ``HipEngine.load_state_dict`` without
        the trainable overlay.  Needs no workspace scratch in any weight format.  Adapters added before stay resident; their
        fingerprints are not checked again."""
        keep = self._load_blocks(sd, prefix, self.arch.layers)
        ts = [self._dev(sd[prefix + k]) for k in ("conv1.weight", "class_embedding", "positional_embedding", "ln_pre.weight",
                                                  "ln_pre.bias", "ln_post.weight", "ln_post.bias", "proj")]
        keep.append(ts)
        _lib.check(self.lib.pevit_load_stem(self._ctx, _lib.stream_ptr(), *[_lib.ptr(t) for t in ts]), "pevit_load_stem")
        torch.cuda.current_stream().synchronize()     # the temporaries above may now be freed
        del keep
        self._backbone_sha256 = adapter_io.backbone_fingerprint(sd, prefix)

    # ------------------------------------------------------------------ adapters
    def add_adapter(self, name: str, ckpt, strict_backbone: bool = True):
        """Make a checkpoint (a path, or the dict ``adapter_io.read_adapter`` returns) resident under ``name``: its flat
        parameter buffer and running statistics go to the device.  Refused (``adapter_io.AdapterError``): another method, LoRA
        rank or arch than this context's, more than ``max_classes`` classes, a head ``pevit_predict`` does not compute
        (``adapter_io.check_servable``), and -- once ``load_backbone`` has run -- a checkpoint trained on another tower
        (``strict_backbone=False``: a warning)."""
        ckpt = adapter_io.read_adapter(ckpt) if isinstance(ckpt, (str, os.PathLike)) else ckpt
        adapter_io.check_adapter(ckpt, method=self.method, lora_rank=self.lora_rank, arch=self.arch, max_classes=self.max_classes,
                                 backbone_sha256=self._backbone_sha256, strict_backbone=strict_backbone)
        adapter_io.check_servable(ckpt)
        t = ckpt["tensors"]
        params = self._dev(adapter_io.flat_params(ckpt))
        C = int(ckpt["meta"]["num_classes"])
        if params.numel() != self.n_tower + C * self.arch.embed_dim + C:
            raise _lib.PevitError(f"host/engine parameter layout mismatch: {params.numel()} floats for {self.n_tower} tower parameters")
        rule = self._dev(t["visual.transformer.phm_rule"]) if self.method == "compacter" else None
        if self._current == name:
            self._current = None         # replaced: select it again
        self._adapters[name] = {"params": params, "running_mean": self._dev(t["channel_bn.running_mean"]),
                                "running_var": self._dev(t["channel_bn.running_var"]), "phm_rule": rule, "num_classes": C,
                                "meta": dict(ckpt["meta"])}

    def use(self, name: str):
        """Select a resident adapter: one pointer swap in the context (``pevit_set_infer_params``; Compacter: plus a 256-byte copy
        of its frozen rule into the arena, enqueued on the current stream).  No synchronise."""
        if name not in self._adapters:
            raise KeyError(f"no adapter {name!r}; resident: {self.adapters()}")
        a = self._adapters[name]
        _lib.check(self.lib.pevit_set_infer_params(self._ctx, _lib.ptr(a["params"]), a["num_classes"]), "pevit_set_infer_params")
        if a["phm_rule"] is not None:
            _lib.check(self.lib.pevit_load_phm_rule(self._ctx, _lib.stream_ptr(), _lib.ptr(a["phm_rule"])), "pevit_load_phm_rule")
        self._current = name

    def adapters(self) -> list:
        return list(self._adapters)

    def drop(self, name: str):
        """Remove a resident adapter; dropping the selected one leaves none selected."""
        if name not in self._adapters:
            raise KeyError(f"no adapter {name!r}; resident: {self.adapters()}")
        if self._current == name:
            self._current = None
        torch.cuda.current_stream(self.device).synchronize()      # (a walk in flight may still read its buffers)
        del self._adapters[name]

    def adapter_meta(self, name: str) -> dict:
        return dict(self._adapters[name]["meta"])

    def _selected(self, who: str, needed: bool = True):
        if self._current is None:
            if needed:
                raise _lib.PevitError(f"{who}: no adapter selected (add_adapter, then use); resident: {self.adapters()}")
            return None
        return self._adapters[self._current]

    # ------------------------------------------------------------------ what the C ABI's raw pointers may read
    def _check_bound(self, B):
        if B > self.max_batch:
            raise _lib.PevitError(f"batch {B} exceeds max_batch {self.max_batch} of this context (predict splits plain tensors itself; "
                                  "a ragged batch must fit)")

    def _chunks(self, images):
        """(lo, hi, pixels as the engine reads them) for every ``max_batch`` images: uint8 pixels through the input helper
        ``HipEngine`` uses (normalised in the patch gather, resized first where ``set_input_resize`` is on), anything else as f32."""
        n = len(images)
        if n < 1:
            raise _lib.PevitError("an empty batch")
        R = self.arch.resolution
        for lo in range(0, n, self.max_batch) if torch.is_tensor(images) else (0,):
            part = images[lo:lo + self.max_batch] if torch.is_tensor(images) else images
            img = self._pixels(part)
            u8 = img.dtype == torch.uint8 and self._input_norm is not None
            if not self._fits(img, torch.uint8 if u8 else torch.float32, (None, 3, R, R)):
                self._refuse(img, f"images must be a contiguous float32 tensor (B,3,{R},{R})", " (or uint8 after set_input_normalization)")
            self._check_bound(img.shape[0])
            yield lo, lo + img.shape[0], img

    def _empty(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    def _out_or_new(self, t, shape):
        if t is None:
            return self._empty(*shape)
        if not self._fits(t, torch.float32, tuple(shape)):
            self._refuse(t, f"output buffer must be a contiguous float32 tensor {tuple(shape)}")
        return t

    def _entry(self, name, img):
        return getattr(self.lib, name + "_u8" if img.dtype == torch.uint8 else name)

    # ------------------------------------------------------------------ images in
    def predict(self, images: torch.Tensor, logits_out=None, return_features: bool = False):
        """images -> logits (n, C) of the selected adapter, C its class count: ``HipEngine.predict`` bit for bit, for ANY number
        of images -- more than ``max_batch`` run in chunks of ``max_batch``, each one ``pevit_predict`` call.  Returns device
        tensors without synchronising; ``(logits, features (n, D))`` with ``return_features``."""
        a = self._selected("predict")
        n, D = len(images), self.arch.embed_dim
        logits = self._out_or_new(logits_out, (n, a["num_classes"]))
        feat = self._empty(n, D) if return_features else None
        for lo, hi, img in self._chunks(images):
            _lib.check(self._entry("pevit_predict", img)(
                self._ctx, _lib.stream_ptr(), _lib.ptr(img), _lib.ptr(a["running_mean"]), _lib.ptr(a["running_var"]),
                _lib.ptr(logits[lo:hi]), _lib.ptr(None if feat is None else feat[lo:hi]), hi - lo), "pevit_predict")
        return (logits, feat) if return_features else logits

    def encode_image(self, images: torch.Tensor) -> torch.Tensor:
        """images -> features (n, D) without a head (``HipEngine.encode_image``).  A ``"none"`` context needs no adapter."""
        self._selected("encode_image", needed=self.method != "none")
        feat = self._empty(len(images), self.arch.embed_dim)
        for lo, hi, img in self._chunks(images):
            _lib.check(self._entry("pevit_encode_image", img)(self._ctx, _lib.stream_ptr(), _lib.ptr(img), _lib.ptr(feat[lo:hi]), hi - lo),
                       "pevit_encode_image")
        return feat

    def zeroshot(self, images: torch.Tensor, text_cd: torch.Tensor, scale: float = 100.0, probs_out=None,
                 return_logits: bool = False, return_features: bool = False):
        """images -> zero-shot class probabilities, as ``HipEngine.zeroshot``: ``text_cd`` contiguous f32 (C, D), class-major
        unit rows, C independent of ``max_classes``."""
        D = self.arch.embed_dim
        if not self._fits(text_cd, torch.float32, (None, D)):
            self._refuse(text_cd, f"text_cd must be a contiguous float32 tensor (C, {D})")
        self._selected("zeroshot", needed=self.method != "none")
        n, Cc = len(images), text_cd.shape[0]
        probs = self._out_or_new(probs_out, (n, Cc))
        logits = self._empty(n, Cc) if return_logits else None
        feat = self._empty(n, D) if return_features else None
        for lo, hi, img in self._chunks(images):
            _lib.check(self._entry("pevit_zeroshot", img)(
                self._ctx, _lib.stream_ptr(), _lib.ptr(img), _lib.ptr(text_cd), Cc, float(scale), _lib.ptr(probs[lo:hi]),
                _lib.ptr(None if logits is None else logits[lo:hi]), _lib.ptr(None if feat is None else feat[lo:hi]), hi - lo),
                "pevit_zeroshot")
        out = (probs,) + ((logits,) if return_logits else ()) + ((feat,) if return_features else ())
        return out if len(out) > 1 else probs

    def tune(self, key: str, value: int) -> int:
        """A/B-measurement knob of THIS context (include/pevit_hip.h: pevit_tune)."""
        return self.lib.pevit_tune(self._ctx, key.encode(), int(value))
