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

With ``slots=2..8`` (``pevit_infer_create_slots`` / ``pevit_infer_create_slots_all``, include/pevit_segments.h and
pevit_segments_all.h; all four methods, in bf16) requests for different
resident adapters are answered in ONE walk of the tower, each as ``use(name); predict(images)`` would answer it alone::

    eng = InferenceEngine(arch, "kadaptation", max_classes=100, max_batch=128, slots=8)
    ...
    a, b = eng.predict_segments([("cifar100", images_a), ("pets", images_b)])
    logits = eng.predict_mixed(images, names)       # one name per image
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib, adapter_io
from ._context import EngineContext
from .engine_input import InputMixin
from .synth import VitArch


# ---- the pure parts of the segmented calls: no tensor, no engine --------------------------------------------------------------------
def group_rows(names):
    """One name per row -> ``(order, groups)``: ``order`` lists the row indices grouped by name, groups in the order of each name's
    first row and rows in their own order inside a group (a stable sort); ``groups`` is ``[(name, count), ...]`` in that order."""
    rows = {}
    for i, n in enumerate(names):
        rows.setdefault(n, []).append(i)
    return [i for r in rows.values() for i in r], [(n, len(r)) for n, r in rows.items()]


def chunk_requests(counts, max_batch):
    """Request sizes -> lists of consecutive request indices, each list one engine call of at most ``max_batch`` images and
    ``_lib.MAX_SEGMENTS`` requests; a request is never split, so one larger than ``max_batch`` is refused."""
    calls, fill = [], max_batch + 1
    for i, n in enumerate(counts):
        if n < 1:
            raise _lib.PevitError(f"request {i}: an empty batch")
        if n > max_batch:
            raise _lib.PevitError(f"request {i}: batch {n} exceeds max_batch {max_batch} of this context (a request is one batch for "
                                  "the raw reshape of its adapter and is not split)")
        if fill + n > max_batch or len(calls[-1]) == _lib.MAX_SEGMENTS:
            calls.append([])
            fill = 0
        calls[-1].append(i)
        fill += n
    return calls


def assign_slots(slot_names, slot_used, clock, wanted):
    """The least-recently-used slot map.  ``slot_names[s]`` is the adapter resident in slot s (None: empty), ``slot_used[s]`` the
    clock of its last use; ``wanted`` the distinct names of one engine call.  Returns ``(slot of every wanted name, [(slot, name)]
    to load, the new clock)`` and updates both lists: a resident name keeps its slot (no load), a missing one takes an empty slot or
    evicts the one used longest ago that this call does not want.  More names than slots: ``PevitError``."""
    if len(set(wanted)) != len(wanted):
        raise ValueError("assign_slots takes distinct names")
    if len(wanted) > len(slot_names):
        raise _lib.PevitError(f"{len(wanted)} adapters in one call on a context of {len(slot_names)} slots: {list(wanted)}")
    clock += 1
    slot_of, loads = {}, []
    for n in wanted:
        if n in slot_names:
            slot_of[n] = slot_names.index(n)
    for n in wanted:
        if n not in slot_of:
            free = [s for s in range(len(slot_names)) if slot_names[s] not in wanted]
            s = min(free, key=lambda s: (slot_names[s] is not None, slot_used[s], s))
            slot_names[s] = n
            slot_of[n] = s
            loads.append((s, n))
    for n in wanted:
        slot_used[slot_of[n]] = clock
    return slot_of, loads, clock


def scatter_rows(order, groups, outs, fill=float("-inf")):
    """Back from the grouped order: ``outs[g]`` is the (count_g, C_g) result of group g; returns (n, max C) with row ``order[j]`` =
    row j of the concatenated groups and ``fill`` in the columns behind a row's class count."""
    width = max(o.shape[1] for o in outs)
    full = outs[0].new_full((len(order), width), fill)
    lo = 0
    for (_, count), o in zip(groups, outs):
        idx = torch.as_tensor(order[lo:lo + count], dtype=torch.long, device=o.device)
        full[idx, :o.shape[1]] = o
        lo += count
    return full


class InferenceEngine(EngineContext, InputMixin):
    """One inference-only context.  All of its state -- also what ``InputMixin`` rebinds -- is declared in ``__init__``."""

    def __init__(self, arch: VitArch, method: str, max_classes: int, max_batch: int, lora_rank: int = 4,
                 device: str | torch.device = "cuda:0", weight_format: str = "bf16", slots: int = 1):
        super().__init__(device)
        self.arch, self.method, self.max_classes, self.lora_rank, self.max_batch = arch, method, int(max_classes), lora_rank, int(max_batch)
        if weight_format not in _lib.WEIGHT_FORMATS:
            raise ValueError(f"weight_format {weight_format!r}: expected one of {sorted(_lib.WEIGHT_FORMATS)}")
        self.weight_format = weight_format
        dims = _lib.PevitDims(arch.width, arch.layers, arch.patch, arch.resolution, arch.embed_dim,
                              _lib.METHOD_IDS[method], lora_rank, self.max_classes, _lib.WEIGHT_FORMATS[weight_format])
        self.slots = int(slots)          # > 1: adapter slots for predict_segments / predict_mixed (pevit_infer_create_slots)
        if self.slots > 1:
            self._create_slots(dims)
        else:
            self._create("pevit_infer_create", dims, self.max_batch)
        self.n_tower = self.lib.pevit_num_tower_params(self._ctx)
        self._adapters = {}              # name -> {"params", "running_mean", "running_var", "phm_rule" (device), "num_classes", "meta"}
        self._current = None             # the name ``use`` selected
        self._slot_names = [None] * (self.slots if self.slots > 1 else 0)    # the adapter resident in every slot
        self._slot_used = [0] * len(self._slot_names)                        # ... and the clock of its last use (assign_slots)
        self._slot_clock = 0
        self._backbone_sha256 = None     # adapter_io.backbone_fingerprint of the tower load_backbone read
        # ---- engine_input.py
        self._input_norm = None          # (mean, std) once set_input_normalization has run: uint8 batches are taken from then on
        self._input_resize, self._resize_center_crop = False, True       # set_input_resize(on, center_crop)
        self._resize_buf, self._resize_cache = None, {}  # resize_u8: its staging (on first use), (h, w, crop) -> device tables

    def _create_slots(self, dims):
        """``EngineContext._create`` through the entry that takes a slot count: the post-MLP methods through
        ``pevit_infer_create_slots_all`` (include/pevit_segments_all.h), the attention-site methods through the entry they always used."""
        entry = "pevit_infer_create_slots_all" if self.method in ("adapter", "compacter") else "pevit_infer_create_slots"
        _lib.check(getattr(self.lib, entry)(C.byref(dims), self.slots, C.byref(self._ctx)), entry)
        self.arena = torch.zeros(self.lib.pevit_arena_bytes(self._ctx), dtype=torch.uint8, device=self.device)
        self._bind(self.max_batch)

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
        self._slot_names[:] = [None] * len(self._slot_names)      # (pevit_load_block emptied every slot)

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
        self._forget_slot(name)
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
        self._forget_slot(name)
        torch.cuda.current_stream(self.device).synchronize()      # (a walk in flight may still read its buffers)
        del self._adapters[name]

    def _forget_slot(self, name):
        """The slot that holds ``name`` (if any) is empty from here on: the next segmented call that wants the name loads it again."""
        if name in self._slot_names:
            if name in self._adapters:
                torch.cuda.current_stream(self.device).synchronize()      # (a segmented walk in flight may still read the old buffer)
            self._slot_names[self._slot_names.index(name)] = None

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

    # ------------------------------------------------------------------ requests for several adapters in one walk
    def _load_slot(self, slot, name):
        a = self._adapters[name]
        if a["phm_rule"] is not None:       # Compacter: the slot's frozen rule, read while its panels are built
            _lib.check(self.lib.pevit_load_adapter_slot_rule(self._ctx, _lib.stream_ptr(), slot, _lib.ptr(a["params"]), a["num_classes"],
                                                             _lib.ptr(a["phm_rule"])), "pevit_load_adapter_slot_rule")
            return
        _lib.check(self.lib.pevit_load_adapter_slot(self._ctx, _lib.stream_ptr(), slot, _lib.ptr(a["params"]), a["num_classes"]),
                   "pevit_load_adapter_slot")

    def _segments_call(self, img, parts):
        """One ``pevit_predict_segments`` call: ``img`` the concatenated pixels, ``parts`` = [(slot, adapter, count, logits, features)]."""
        segs = (_lib.PevitSegment * len(parts))()
        first = 0
        for g, (slot, a, count, logits, feat) in zip(segs, parts):
            g.first, g.count, g.slot = first, count, slot
            g.running_mean, g.running_var = a["running_mean"].data_ptr(), a["running_var"].data_ptr()
            g.logits, g.features = logits.data_ptr(), None if feat is None else feat.data_ptr()
            first += count
        _lib.check(self._entry("pevit_predict_segments", img)(self._ctx, _lib.stream_ptr(), _lib.ptr(img), first, len(parts), segs),
                   "pevit_predict_segments")

    def _request_pixels(self, images, alone):
        """``_pixels`` of one request.  A native-size uint8 request comes back from the input resize as a view of the ONE staging
        tensor, which the next request's resize overwrites: unless the request is ``alone`` in its engine call it is copied out
        (on the stream, behind its resize launch) before the next one is resized."""
        p = self._pixels(images)
        return p.clone() if not alone and self._needs_resize(images) else p

    def predict_segments(self, requests, return_features: bool = False):
        """``requests = [(name, images), ...]`` -> one logits tensor (count, C_name) per request, in request order: requests for
        DIFFERENT resident adapters answered in one walk of the tower (``pevit_predict_segments``), on a context created with
        ``slots > 1``.  Each request is answered as ``use(name); predict(images)`` would answer it alone -- it is one batch for the
        raw reshape of its adapter, whoever shares the call with it.  The requests are concatenated on the device and run in calls of
        at most ``max_batch`` images; a request is never split, so one larger than ``max_batch`` is refused.  Adapters go to slots
        by least-recently-used, and a slot is loaded only when its adapter is not resident in one; more distinct names in one
        call than slots is refused.  Pixels as ``predict`` takes them -- f32, or uint8 after ``set_input_normalization``, of native
        size with ``set_input_resize`` (each request is resized on its own and copied out of the staging tensor) -- but all requests
        of a call of one kind, and tensors only: a ragged batch is refused.  No synchronise; ``[(logits, features (count, D)),
        ...]`` with ``return_features``."""
        if self.slots < 2:
            raise _lib.PevitError("predict_segments needs a context with adapter slots: InferenceEngine(..., slots=2..8)")
        requests = list(requests)
        for name, _ in requests:
            if name not in self._adapters:
                raise KeyError(f"no adapter {name!r}; resident: {self.adapters()}")
        wanted = list(dict.fromkeys(name for name, _ in requests))
        if len(wanted) > self.slots:
            raise _lib.PevitError(f"{len(wanted)} adapters in one call on a context of {self.slots} slots: {wanted}")
        for i, (_, images) in enumerate(requests):
            if not torch.is_tensor(images):
                raise _lib.PevitError(f"request {i}: predict_segments takes tensors; a ragged batch ({type(images).__name__}) is served "
                                      "by use + predict")
        if len({images.dtype == torch.uint8 for _, images in requests}) > 1:
            raise _lib.PevitError("predict_segments: uint8 and float requests in one call; the requests of a call share one entry point")
        calls = chunk_requests([len(img) for _, img in requests], self.max_batch)
        R, D, out = self.arch.resolution, self.arch.embed_dim, [None] * len(requests)
        for call in calls:
            pix = [self._request_pixels(requests[i][1], alone=len(call) == 1) for i in call]
            u8 = pix[0].dtype == torch.uint8 and self._input_norm is not None
            for p in pix:
                if not self._fits(p, torch.uint8 if u8 else torch.float32, (None, 3, R, R)):
                    self._refuse(p, f"images must be a contiguous float32 tensor (B,3,{R},{R})", " (or uint8 after set_input_normalization)")
            img = pix[0] if len(pix) == 1 else torch.cat(pix)
            slot_of, loads, self._slot_clock = assign_slots(self._slot_names, self._slot_used, self._slot_clock,
                                                            list(dict.fromkeys(requests[i][0] for i in call)))
            for k, (slot, name) in enumerate(loads):
                try:
                    self._load_slot(slot, name)
                except Exception:
                    for s, _ in loads[k:]:            # the library emptied the slot it could not load; the ones behind it never ran
                        self._slot_names[s] = None
                    raise
            parts = []
            for i, p in zip(call, pix):
                a = self._adapters[requests[i][0]]
                logits, feat = self._empty(len(p), a["num_classes"]), self._empty(len(p), D) if return_features else None
                out[i] = (logits, feat) if return_features else logits
                parts.append((slot_of[requests[i][0]], a, len(p), logits, feat))
            self._segments_call(img, parts)
        return out

    def predict_mixed(self, images: torch.Tensor, names):
        """One adapter name per image -> logits (n, C_max), C_max the largest class count among the names, ``-inf`` in the columns
        behind a row's own class count.  The rows are grouped by name (a stable sort: groups in the order of each name's first row)
        and run through ``predict_segments``, then scattered back into the order they came in.
        EACH NAME'S ROWS FORM ONE BATCH for the raw reshape of the adapter delta: a row's logits are those of ``use(name);
        predict(all rows of that name, in their order)`` -- they depend on the other rows of the SAME name in this call, as an
        image's logits depend on its batch in ``predict``, and on no row of another name.  That is the attention-site methods
        (KAdaptation, LoRA); the post-MLP methods (Adapter, Compacter) are row-wise and have no raw reshape: there a row's logits
        depend on no other row."""
        names = list(names)
        if not torch.is_tensor(images):
            raise _lib.PevitError(f"predict_mixed takes one tensor of images; a ragged batch ({type(images).__name__}) is served by use + predict")
        if len(names) != len(images) or not names:
            raise _lib.PevitError(f"predict_mixed: {len(names)} names for {len(images)} images")
        order, groups = group_rows(names)
        grouped = images[torch.as_tensor(order, dtype=torch.long, device=images.device)]
        requests, lo = [], 0
        for name, count in groups:
            requests.append((name, grouped[lo:lo + count]))
            lo += count
        return scatter_rows(order, groups, self.predict_segments(requests))

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
