"""Host-side owner of one HIP engine context (one per process / GPU).

PyTorch is used here for what it is good at -- device memory, streams, the
``torch.distributed`` collective on the flat gradient buffer -- while every
FLOP of the fine-tune step runs in ``libpevit_hip.so`` (include/pevit_hip.h).
The trainable parameters live in ONE flat f32 buffer in the reference's
``named_parameters()`` order (adapters, then ``layers.0.weight/bias`` of the
Classifier head, kadaptation_clip.py:132); ``param_views()`` exposes them under
the reference's names so that state-dicts, the requires_grad-by-substring rule
and DP all-reduce see exactly the tensors the reference has.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from collections import OrderedDict

import torch

from . import _lib, dp
from .preprocess import RaggedBatch
from .synth import VitArch

PHM_DIM_KADAPT = 32     # model.py:485
BOTTLENECK = 64         # adapter_model.py:305, compacter_model.py:472
PHM_DIM_COMPACTER = 4   # compacter_model.py:512


def adapter_param_spec(method: str, width: int, layers: int, lora_rank: int = 4):
    """(name, shape, trainable) of the tensors the reference adds to the OpenAI layout, in the
    reference's ``named_parameters()`` order (verified against the golden
    fixtures' name lists in tests/test_host_api.py)."""
    E, t = width, "visual.transformer."
    out = []
    if method == "kadaptation":
        n = PHM_DIM_KADAPT
        out += [(t + "phm_rule1_left", (n, n, 1), True), (t + "phm_rule1_right", (n, 1, n), True),
                (t + "phm_rule2_left", (n, n, 1), True), (t + "phm_rule2_right", (n, 1, n), True)]
        for i in range(layers):
            a = f"{t}resblocks.{i}.attn."
            out += [(a + "q_proj_adapter1_left", (n, E // n, 1), True), (a + "q_proj_adapter1_right", (n, 1, E // n), True),
                    (a + "v_proj_adapter1_left", (n, E // n, 1), True), (a + "v_proj_adapter1_right", (n, 1, E // n), True),
                    (a + "b", (E,), True)]
    elif method == "lora":
        for i in range(layers):
            a = f"{t}resblocks.{i}.attn."
            out += [(a + "q_proj_adapter1.weight", (lora_rank, E), True), (a + "q_proj_adapter2.weight", (E, lora_rank), True),
                    (a + "v_proj_adapter1.weight", (lora_rank, E), True), (a + "v_proj_adapter2.weight", (E, lora_rank), True)]
    elif method == "adapter":
        for i in range(layers):
            a = f"{t}resblocks.{i}.adapter."
            out += [(a + "adapter_norm_before.weight", (E,), True), (a + "adapter_norm_before.bias", (E,), True),
                    (a + "adapter_down.1.weight", (BOTTLENECK, E), True), (a + "adapter_down.1.bias", (BOTTLENECK,), True),
                    (a + "adapter_up.weight", (E, BOTTLENECK), True), (a + "adapter_up.bias", (E,), True)]
    elif method == "compacter":
        n = PHM_DIM_COMPACTER
        out += [(t + "phm_rule", (n, n, n), False)]          # name lacks 'compacter' -> frozen (compacter_clip.py:122)
        for i in range(layers):
            a = f"{t}resblocks.{i}.compacter."
            out += [(a + "adapter_norm_before.weight", (E,), True), (a + "adapter_norm_before.bias", (E,), True),
                    (a + "adapter_down.1.W_left", (n, E // n, 1), True), (a + "adapter_down.1.W_right", (n, 1, BOTTLENECK // n), True),
                    (a + "adapter_down.1.b", (BOTTLENECK,), True),
                    (a + "adapter_up.W_left", (n, BOTTLENECK // n, 1), True), (a + "adapter_up.W_right", (n, 1, E // n), True),
                    (a + "adapter_up.b", (E,), True)]
    elif method == "none":
        pass
    else:
        raise ValueError(f"unknown PEFT method {method!r}")
    return out


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


@dataclasses.dataclass
class OptimPlan:
    """What ``HipEngine.optimizer_step`` needs to run a torch optimizer's ``step()`` as one launch over the flat buffer.

    ``kind``: "sgd" | "adam" | "adamw".  ``groups``: one dict per LIVE parameter group, in ``group_of``'s numbering, with ``lr``,
    ``weight_decay`` and (SGD) ``momentum``, ``nesterov`` / (Adam kinds) ``beta1``, ``beta2``, ``eps`` as Python floats.
    ``group_of``: host uint8 tensor over the flat buffer, 255 where the parameter's ``.grad`` is None (it is uploaded only when
    its contents change: a tensor edited in place with torch operations is compared again, one written through a NumPy view or
    a raw pointer is not, so build a new tensor for those).  ``group_index``: the position of each live group in the torch optimizer's ``param_groups``
    (``refresh`` re-reads the hyper-parameters from there, so schedulers keep working)."""
    kind: str
    groups: list
    group_of: torch.Tensor
    group_index: list = dataclasses.field(default_factory=list)

    def refresh(self, optimizer):
        for k, j in enumerate(self.group_index):
            self.groups[k] = _group_hypers(self.kind, optimizer.param_groups[j])
        return self


def _group_hypers(kind, g):
    if kind == "sgd":
        return {"lr": float(g["lr"]), "weight_decay": float(g["weight_decay"]), "momentum": float(g["momentum"]),
                "nesterov": bool(g["nesterov"])}
    return {"lr": float(g["lr"]), "weight_decay": float(g["weight_decay"]), "beta1": float(g["betas"][0]),
            "beta2": float(g["betas"][1]), "eps": float(g["eps"])}


class HipEngine:
    def __init__(self, arch: VitArch, method: str, num_classes: int, max_batch: int, lora_rank: int = 4,
                 device: str | torch.device = "cuda:0", weight_format: str = "bf16"):
        if not torch.cuda.is_available():
            raise _lib.PevitError("HipEngine needs a ROCm GPU (gfx950); there is no CPU fallback")
        self.lib = _lib.load()
        self.arch, self.method, self.num_classes = arch, method, num_classes
        self.lora_rank, self.max_batch = lora_rank, max_batch
        if weight_format not in _lib.WEIGHT_FORMATS:
            raise ValueError(f"weight_format {weight_format!r}: expected one of {sorted(_lib.WEIGHT_FORMATS)}")
        self.weight_format = weight_format
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        dims = _lib.PevitDims(arch.width, arch.layers, arch.patch, arch.resolution, arch.embed_dim,
                              _lib.METHOD_IDS[method], lora_rank, num_classes, _lib.WEIGHT_FORMATS[weight_format])
        self._ctx = C.c_void_p()
        _lib.check(self.lib.pevit_ctx_create(C.byref(dims), C.byref(self._ctx)), "pevit_ctx_create")
        self.arena = torch.zeros(self.lib.pevit_arena_bytes(self._ctx), dtype=torch.uint8, device=self.device)
        self.workspace = torch.empty(self.lib.pevit_workspace_bytes(self._ctx, max_batch), dtype=torch.uint8,
                                     device=self.device)
        _lib.check(self.lib.pevit_bind(self._ctx, _lib.ptr(self.arena), self.arena.numel(), _lib.ptr(self.workspace),
                                       self.workspace.numel(), max_batch), "pevit_bind")
        self.n_tower = self.lib.pevit_num_tower_params(self._ctx)
        self.n_params = self.lib.pevit_num_params(self._ctx)
        self.params = torch.zeros(self.n_params, dtype=torch.float32, device=self.device)
        self.grads = torch.zeros_like(self.params)
        self.momentum = torch.zeros_like(self.params)
        mask = (C.c_ubyte * self.n_params)()
        _lib.check(self.lib.pevit_param_grad_mask(self._ctx, mask, self.n_params), "pevit_param_grad_mask")
        self.grad_mask_host = torch.frombuffer(bytearray(mask), dtype=torch.uint8).clone()
        self.grad_mask = self.grad_mask_host.to(self.device)
        _lib.check(self.lib.pevit_set_params(self._ctx, _lib.ptr(self.params), _lib.ptr(self.grads),
                                             _lib.ptr(self.momentum), _lib.ptr(self.grad_mask)), "pevit_set_params")
        # BatchNorm1d(D, affine=False) buffers of the Classifier (kadaptation_clip.py:128-131)
        self.running_mean = torch.zeros(arch.embed_dim, dtype=torch.float32, device=self.device)
        self.running_var = torch.ones(arch.embed_dim, dtype=torch.float32, device=self.device)
        self._spec = [(n, s) for n, s, tr in adapter_param_spec(method, arch.width, arch.layers, lora_rank) if tr]
        total = sum(_numel(s) for _, s in self._spec)
        if total != self.n_tower:
            raise _lib.PevitError(f"host/engine parameter layout mismatch: {total} vs {self.n_tower}")
        self._steps = 0
        self.exp_avg_sq = None           # Adam / AdamW second moment: allocated on first use (optimizer_step); exp_avg is self.momentum
        self._group_of = None            # device copy of the last OptimPlan.group_of ...
        self._group_of_host = None       # ... a host copy of what was uploaded ...
        self._group_of_seen = None       # ... and the (tensor, version) last compared with it: an in-place edit of a plan is seen
        self._optim_kind = None          # which optimizer the momentum / exp_avg_sq buffers belong to (None: fresh, or plain sgd_step)
        self.forward_generation = 0      # bumped by EVERY forward: each one overwrites the single activation workspace
        self.block_generation = {}       # per block: bumped by every forward THROUGH that block (blocks keep their own activations)
        self.attention_generation = {}   # per block: the block_generation its last attention_forward left (attention seam)
        self._logits = torch.empty((max_batch, num_classes), dtype=torch.float32, device=self.device)
        self._loss = torch.zeros(1, dtype=torch.float32, device=self.device)

    def __del__(self):
        try:
            if getattr(self, "_ctx", None):
                self.lib.pevit_ctx_destroy(self._ctx)
                self._ctx = None
        except Exception:
            pass

    def tune(self, key: str, value: int) -> int:
        """A/B-measurement knob of THIS context (include/pevit_hip.h: pevit_tune)."""
        return self.lib.pevit_tune(self._ctx, key.encode(), int(value))

    def ensure_batch(self, batch: int):
        """Grow the activation workspace so that steps of ``batch`` images fit (re-binds; weights stay)."""
        if batch <= self.max_batch:
            return
        torch.cuda.synchronize(self.device)
        self.workspace = None
        self.workspace = torch.empty(self.lib.pevit_workspace_bytes(self._ctx, batch), dtype=torch.uint8,
                                     device=self.device)
        _lib.check(self.lib.pevit_bind(self._ctx, _lib.ptr(self.arena), self.arena.numel(), _lib.ptr(self.workspace),
                                       self.workspace.numel(), batch), "pevit_bind")
        self._logits = torch.empty((batch, self.num_classes), dtype=torch.float32, device=self.device)
        if getattr(self, "_resize_buf", None) is not None:         # the staging of resize_u8 follows the batch bound
            self._resize_buf = None
            self._resize_buf = self._resize_staging(batch)
        self.max_batch = batch

    # ------------------------------------------------------------------ parameters
    def param_views(self, buf: torch.Tensor | None = None) -> "OrderedDict[str, torch.Tensor]":
        """Views of the flat buffer under the reference's parameter names (+ head).  (Pipelined DP: the current stream first
        waits for the update still running on the second stream -- a checkpoint / state export right behind a step must not read
        half-updated parameters.)"""
        self.dp_flush()
        buf = self.params if buf is None else buf
        out, off = OrderedDict(), 0
        for name, shape in self._spec:
            n = _numel(shape)
            out[name] = buf[off:off + n].view(shape)
            off += n
        D, Cc = self.arch.embed_dim, self.num_classes
        out["layers.0.weight"] = buf[off:off + Cc * D].view(Cc, D); off += Cc * D
        out["layers.0.bias"] = buf[off:off + Cc].view(Cc); off += Cc
        assert off == self.n_params
        return out

    def grad_views(self):
        self.dp_flush()
        return self.param_views(self.grads)

    # ------------------------------------------------------------------ frozen weights
    def load_state_dict(self, sd, prefix: str = "visual."):
        """Frozen backbone from an OpenAI-layout state-dict (any float dtype, any device)."""
        self.dp_flush()
        s = _lib.stream_ptr()

        def dev(key):
            return sd[prefix + key].detach().to(device=self.device, dtype=torch.float32).contiguous()

        keep = []
        for i in range(self.arch.layers):
            b = f"transformer.resblocks.{i}."
            ts = [dev(b + k) for k in ("attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight",
                                       "attn.out_proj.bias", "ln_1.weight", "ln_1.bias", "mlp.c_fc.weight",
                                       "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias", "ln_2.weight", "ln_2.bias")]
            keep.append(ts)
            _lib.check(self.lib.pevit_load_block(self._ctx, s, i, *[_lib.ptr(t) for t in ts]), "pevit_load_block")
        ts = [dev(k) for k in ("conv1.weight", "class_embedding", "positional_embedding", "ln_pre.weight",
                               "ln_pre.bias", "ln_post.weight", "ln_post.bias", "proj")]
        keep.append(ts)
        _lib.check(self.lib.pevit_load_stem(self._ctx, s, *[_lib.ptr(t) for t in ts]), "pevit_load_stem")
        if self.method == "compacter":
            r = dev("transformer.phm_rule"); keep.append([r])
            _lib.check(self.lib.pevit_load_phm_rule(self._ctx, s, _lib.ptr(r)), "pevit_load_phm_rule")
        torch.cuda.current_stream().synchronize()     # the temporaries above may now be freed
        del keep
        self.load_trainable(sd)

    def load_phm_rule(self, rule: torch.Tensor):
        """Compacter's shared, frozen (4,4,4) rule (compacter_model.py:511-519) into the arena."""
        r = rule.detach().to(device=self.device, dtype=torch.float32).contiguous()
        _lib.check(self.lib.pevit_load_phm_rule(self._ctx, _lib.stream_ptr(), _lib.ptr(r)), "pevit_load_phm_rule")
        torch.cuda.current_stream().synchronize()

    def load_trainable(self, sd):
        """Adapter / head tensors present in ``sd`` overlay the current values (model.py:1247-1250)."""
        views = self.param_views()
        with torch.no_grad():
            for name, v in views.items():
                if name in sd:
                    v.copy_(sd[name].to(device=self.device, dtype=torch.float32).view_as(v))

    # ------------------------------------------------------------------ hot path
    def set_input_normalization(self, mean, std):
        """Preprocessing of uint8 batches, x = (u8 / 255 - mean[c]) / std[c] (the reference's ToTensor + Normalize,
        feature.py:537-542 with INPUT.MEAN / INPUT.STD), applied inside the patch gather of the engine."""
        m = (C.c_float * 3)(*[float(v) for v in mean]); sd = (C.c_float * 3)(*[float(v) for v in std])
        _lib.check(self.lib.pevit_set_input_norm(self._ctx, m, sd), "pevit_set_input_norm")
        self._input_norm = (tuple(float(v) for v in mean), tuple(float(v) for v in std))

    # ---- native-size uint8 batches: the reference's Resize(n_px, bicubic) + CenterCrop in one launch (csrc/resize.hip) ----------
    def set_input_resize(self, on: bool = True, center_crop: bool = True):
        """With ``on``, every method that takes uint8 pixels also takes contiguous uint8 (B,3,h,w) of ONE other size per batch --
        the native size of the dataset -- and runs the reference's ``Resize(R, bicubic) + CenterCrop(R)`` (clip_load._Preprocess)
        on the GPU first, bit for bit what Pillow gives (``resize_u8``); the resized batch then takes the unchanged uint8 path.
        Off by default: a uint8 batch of another size than (R,R) is refused.  f32 batches of another size, and uint8 batches before
        ``set_input_normalization``, are refused either way.
        ``center_crop`` False (the reference's ``DATASET.CENTER_CROP False``, feature.py:543-549): ``Resize((R, R))`` instead, the
        whole picture squashed to R x R and nothing cropped.  A ``preprocess.RaggedBatch`` -- every image its own size -- is taken
        like a native-size batch, in one launch of its own kernel; it carries its tables, and so its mode, which must be this one."""
        self._input_resize = bool(on)
        self._resize_center_crop = bool(center_crop)

    def _resize_staging(self, batch):
        R = self.arch.resolution
        return torch.empty((batch, 3, R, R), dtype=torch.uint8, device=self.device)

    def _resize_tables(self, h, w):
        """Device tables of the (h, w) -> (R, R) resize + crop, planned by the library and uploaded once per source size."""
        cache = self.__dict__.setdefault("_resize_cache", {})
        crop = bool(getattr(self, "_resize_center_crop", True))
        if (h, w, crop) not in cache:
            R = self.arch.resolution
            nh, nw, top, left = C.c_int(R), C.c_int(R), C.c_int(0), C.c_int(0)      # DATASET.CENTER_CROP False: squash, no crop
            if crop:
                _lib.check(self.lib.pevit_resize_geometry(h, w, R, C.byref(nh), C.byref(nw), C.byref(top), C.byref(left)),
                           "pevit_resize_geometry")
            out = []
            for in_size, out_size, first in ((w, nw.value, left.value), (h, nh.value, top.value)):
                ks = self.lib.pevit_resize_axis(in_size, out_size, 0, 0, None, None)
                if ks < 1:
                    _lib.check(-1, "pevit_resize_axis")
                if ks > 33 or in_size > 4096 or R > 256:
                    raise _lib.PevitError(f"resize_u8: a {h} x {w} source for a {R} x {R} tower is outside what the kernel takes "
                                          f"(sides up to 4096, a downscale of at most 8x, targets up to 256)")
                k = torch.empty((R, ks), dtype=torch.int32)
                b = torch.empty((R, 2), dtype=torch.int32)
                _lib.check(self.lib.pevit_resize_axis(in_size, out_size, first, R, C.c_void_p(k.data_ptr()), C.c_void_p(b.data_ptr())),
                           "pevit_resize_axis")
                out += [k.to(self.device), b.to(self.device), ks]
            cache[(h, w, crop)] = tuple(out)
        return cache[(h, w, crop)]

    def _resize_ragged(self, batch) -> torch.Tensor:
        """A ``preprocess.RaggedBatch`` on this device -> uint8 (B,3,R,R) in ONE launch (``pevit_resize_ragged_u8``), bit for bit
        ``preprocess.resize_u8`` of every image; a view of the resize staging tensor, like ``resize_u8``'s result."""
        R = self.arch.resolution
        if batch.device != self.device or batch.index.dtype != torch.int64 or not batch.index.is_contiguous() or len(batch) < 1:
            raise _lib.PevitError(f"resize_u8: a ragged batch must live on {self.device} with a contiguous int64 index of at least "
                                  f"one image; got {len(batch)} images on {batch.device}")
        if batch.out != R or batch.center_crop != bool(getattr(self, "_resize_center_crop", True)):
            raise _lib.PevitError(f"resize_u8: the ragged set was planned for a {batch.out} x {batch.out} tower with center_crop="
                                  f"{batch.center_crop}; this engine resizes to {R} x {R} with center_crop="
                                  f"{bool(getattr(self, '_resize_center_crop', True))}")
        B = len(batch)
        if B > self.max_batch:
            raise _lib.PevitError(f"batch {B} exceeds the bound workspace ({self.max_batch}): call ensure_batch")
        if getattr(self, "_resize_buf", None) is None:
            self._resize_buf = self._resize_staging(self.max_batch)
        out = self._resize_buf[:B]
        a = _lib.PevitResizeRaggedArgs(
            pool=_lib.ptr(batch.pool), pool_bytes=batch.pool.numel(), desc=_lib.ptr(batch.desc), k_pool=_lib.ptr(batch.k_pool),
            k_len=batch.k_pool.numel(), b_pool=_lib.ptr(batch.b_pool), b_len=batch.b_pool.numel(), index=_lib.ptr(batch.index),
            dst=_lib.ptr(out), n_images=batch.desc.shape[0], batch=B, out=R, max_ksize_v=batch.max_ksize_v)
        _lib.check(self.lib.pevit_resize_ragged_u8(_lib.stream_ptr(), C.byref(a)), "pevit_resize_ragged_u8")
        return out

    def resize_u8(self, images: torch.Tensor) -> torch.Tensor:
        """uint8 (B,3,h,w) -> uint8 (B,3,R,R): Pillow's bicubic resize of the shorter side to R and the centre crop, in ONE launch
        (``pevit_resize_u8``), bit for bit ``preprocess.resize_center_crop_u8``.  The result is a view of an engine-owned staging
        tensor (``max_batch`` images) that the next call overwrites; no synchronise.  With ``set_input_resize(center_crop=False)``
        the whole picture is squashed to (R,R) instead (``preprocess.resize_u8(..., center_crop=False)``).  A
        ``preprocess.RaggedBatch`` is resized image by image in one launch of ``pevit_resize_ragged_u8``."""
        if isinstance(images, RaggedBatch):
            return self._resize_ragged(images)
        if images.device != self.device or images.dtype != torch.uint8 or not images.is_contiguous() or images.dim() != 4 \
                or images.shape[1] != 3 or images.shape[0] < 1:
            raise _lib.PevitError(f"resize_u8: images must be a contiguous uint8 tensor (B,3,h,w) on {self.device}; got "
                                  f"{tuple(images.shape)} {images.dtype} on {images.device}")
        B, _, h, w = images.shape
        if B > self.max_batch:
            raise _lib.PevitError(f"batch {B} exceeds the bound workspace ({self.max_batch}): call ensure_batch")
        kh, bh, ksh, kv, bv, ksv = self._resize_tables(int(h), int(w))
        if getattr(self, "_resize_buf", None) is None:
            self._resize_buf = self._resize_staging(self.max_batch)
        out = self._resize_buf[:B]
        R = self.arch.resolution
        _lib.check(self.lib.pevit_resize_u8(_lib.stream_ptr(), _lib.ptr(images), 3 * B, h, w, _lib.ptr(out), R, R, _lib.ptr(kh),
                                            _lib.ptr(bh), ksh, _lib.ptr(kv), _lib.ptr(bv), ksv), "pevit_resize_u8")
        return out

    def _needs_resize(self, images) -> bool:
        R = self.arch.resolution
        if isinstance(images, RaggedBatch):
            return True
        return bool(getattr(self, "_input_resize", False)) and getattr(self, "_input_norm", None) is not None \
            and images.dtype == torch.uint8 and images.dim() == 4 and tuple(images.shape[2:]) != (R, R)

    def _input(self, images):
        """The ONE place a native-size uint8 batch becomes (B,3,R,R): every uint8-taking method passes its images through here
        and then through its unchanged checks and its unchanged ``_u8`` entry.  Anything else comes back as it is.  A ragged batch
        (``preprocess.RaggedBatch``) can only be resized: it is refused where a native-size batch would be."""
        if isinstance(images, RaggedBatch) and not (getattr(self, "_input_resize", False) and getattr(self, "_input_norm", None) is not None):
            raise _lib.PevitError("a ragged uint8 batch needs set_input_normalization(mean, std) and set_input_resize(True)")
        return self.resize_u8(images) if self._needs_resize(images) else images

    def _check_batch(self, images, labels=None):
        """The C ABI takes raw pointers: reject anything that is not what it will read (f32 NCHW images -- or uint8 pixels once
        set_input_normalization has been called -- and int64 class indices (B,) or f32 multi-label targets (B, num_classes),
        contiguous, on this engine's device)."""
        a = self.arch
        ok_dtype = images.dtype == torch.float32 or (images.dtype == torch.uint8 and getattr(self, "_input_norm", None) is not None)
        if images.device != self.device or not ok_dtype or not images.is_contiguous() or \
                tuple(images.shape[1:]) != (3, a.resolution, a.resolution):
            raise _lib.PevitError(f"images must be a contiguous float32 tensor (B,3,{a.resolution},{a.resolution}) on {self.device} "
                                  f"(or uint8 after set_input_normalization); got {tuple(images.shape)} {images.dtype} on {images.device}")
        if images.shape[0] > self.max_batch:
            raise _lib.PevitError(f"batch {images.shape[0]} exceeds the bound workspace ({self.max_batch}): call ensure_batch")
        return None if labels is None else self._check_labels(labels, images.shape[0])

    def _check_labels(self, labels, B):
        """True for multi-label targets (BCEWithLogitsLoss), False for class indices (cross-entropy)."""
        if labels.device == self.device and labels.is_contiguous():
            if labels.dtype == torch.int64 and tuple(labels.shape) == (B,):
                return False
            if labels.dtype == torch.float32 and tuple(labels.shape) == (B, self.num_classes):
                return True
        raise _lib.PevitError(f"labels must be a contiguous int64 tensor ({B},) or float32 tensor ({B}, {self.num_classes}) on "
                              f"{self.device}; got {tuple(labels.shape)} {labels.dtype} on {labels.device}")

    def _train_fn(self, images, bce):
        """The fused C entry for this input form: uint8 or f32 pixels x cross-entropy or BCE."""
        if images.dtype == torch.uint8:
            return self.lib.pevit_train_forward_backward_bce_u8 if bce else self.lib.pevit_train_forward_backward_u8
        return self.lib.pevit_train_forward_backward_bce if bce else self.lib.pevit_train_forward_backward

    def _head_fn(self, labels, B):
        return self.lib.pevit_head_forward_backward_bce if self._check_labels(labels, B) else self.lib.pevit_head_forward_backward

    def transformer_forward(self, x_nbe: torch.Tensor, save: bool = True) -> torch.Tensor:
        self.dp_flush()
        N, B, E = x_nbe.shape
        if (N, E) != (self.arch.tokens, self.arch.width) or x_nbe.device != self.device:
            raise _lib.PevitError(f"transformer_forward expects ({self.arch.tokens}, B, {self.arch.width}) on {self.device}, "
                                  f"got {tuple(x_nbe.shape)} on {x_nbe.device}")
        self.forward_generation += 1
        for l in range(self.arch.layers):
            self.block_generation[l] = self.block_generation.get(l, 0) + 1
        x = x_nbe.contiguous().float()
        y = torch.empty_like(x)
        _lib.check(self.lib.pevit_transformer_forward(self._ctx, _lib.stream_ptr(), _lib.ptr(x), _lib.ptr(y), B, int(save)),
                   "pevit_transformer_forward")
        return y

    def blocks_forward(self, x_nbe: torch.Tensor, l_lo: int, l_hi: int, save: bool = True) -> torch.Tensor:
        """Blocks [l_lo, l_hi) on (N,B,E) activations (the reference's ResidualAttentionBlock.forward for one block)."""
        self.dp_flush()
        N, B, E = x_nbe.shape
        if (N, E) != (self.arch.tokens, self.arch.width) or x_nbe.device != self.device:
            raise _lib.PevitError(f"blocks_forward expects ({self.arch.tokens}, B, {self.arch.width}) on {self.device}")
        # every forward -- also one through a few blocks -- overwrites activations a pending whole-tower backward would read;
        # the output of block l_hi - 1 also lands in the saved INPUT of block l_hi
        self.forward_generation += 1
        for l in range(l_lo, min(l_hi + 1, self.arch.layers)):
            self.block_generation[l] = self.block_generation.get(l, 0) + 1
        x = x_nbe.contiguous().float()
        y = torch.empty_like(x)
        _lib.check(self.lib.pevit_blocks_forward(self._ctx, _lib.stream_ptr(), _lib.ptr(x), _lib.ptr(y), B, int(save), l_lo, l_hi),
                   "pevit_blocks_forward")
        return y

    def blocks_backward(self, dy_nbe: torch.Tensor, l_lo: int, l_hi: int, need_dx: bool = True):
        self.dp_flush()
        N, B, E = dy_nbe.shape
        dy = dy_nbe.contiguous().float()
        dx = torch.empty_like(dy) if need_dx else None
        _lib.check(self.lib.pevit_blocks_backward(self._ctx, _lib.stream_ptr(), _lib.ptr(dy), _lib.ptr(dx), B, l_lo, l_hi),
                   "pevit_blocks_backward")
        return dx

    def attention_forward(self, x_nbe: torch.Tensor, layer: int, save: bool = True, weights: str | None = None):
        """MultiheadAttention.forward(x, x, x) of block ``layer`` (the reference's resblocks[layer].attn, model.py:837-944) on the
        attention INPUT x (N,B,E): returns (out_proj output without the residual, weights or None).  ``weights``: None
        (need_weights=False), "mean" ((B,N,N) head average) or "heads" ((B,H,N,N))."""
        self.dp_flush()
        N, B, E = x_nbe.shape
        if (N, E) != (self.arch.tokens, self.arch.width) or x_nbe.device != self.device:
            raise _lib.PevitError(f"attention_forward expects ({self.arch.tokens}, B, {self.arch.width}) on {self.device}, "
                                  f"got {tuple(x_nbe.shape)} on {x_nbe.device}")
        if not 0 <= layer < self.arch.layers:
            raise _lib.PevitError(f"attention_forward: layer {layer} outside [0, {self.arch.layers})")
        if weights not in (None, "mean", "heads"):
            raise ValueError(f"weights={weights!r}: expected None, 'mean' or 'heads'")
        # the seam's activations live in the layer's saved slots: a pending backward through the tower or through this block is
        # no longer possible
        self.forward_generation += 1
        self.block_generation[layer] = self.block_generation.get(layer, 0) + 1
        self.attention_generation[layer] = self.block_generation[layer]
        x = x_nbe.contiguous().float()
        y = torch.empty_like(x)
        w = None
        if weights == "mean":
            w = torch.empty((B, N, N), dtype=torch.float32, device=self.device)
        elif weights == "heads":
            w = torch.empty((B, self.arch.heads, N, N), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pevit_attention_forward(self._ctx, _lib.stream_ptr(), layer, _lib.ptr(x), _lib.ptr(y), B, int(save),
                                                    _lib.ptr(w), int(weights != "heads")), "pevit_attention_forward")
        return y, w

    def attention_backward(self, dy_nbe: torch.Tensor, layer: int, need_dx: bool = True):
        """dy (N,B,E) of the attention output -> dx of its input; accumulates the adapter gradients of ``layer`` into ``grads``."""
        self.dp_flush()
        N, B, E = dy_nbe.shape
        dy = dy_nbe.contiguous().float()
        dx = torch.empty_like(dy) if need_dx else None
        _lib.check(self.lib.pevit_attention_backward(self._ctx, _lib.stream_ptr(), layer, _lib.ptr(dy), _lib.ptr(dx), B),
                   "pevit_attention_backward")
        return dx

    def transformer_backward(self, dy_nbe: torch.Tensor, need_dx: bool = True):
        self.dp_flush()
        N, B, E = dy_nbe.shape
        dy = dy_nbe.contiguous().float()
        dx = torch.empty_like(dy) if need_dx else None
        _lib.check(self.lib.pevit_transformer_backward(self._ctx, _lib.stream_ptr(), _lib.ptr(dy), _lib.ptr(dx), B),
                   "pevit_transformer_backward")
        return dx

    def visual_forward(self, images: torch.Tensor, save: bool = True) -> torch.Tensor:
        self.dp_flush()
        B = images.shape[0]
        img = self._input(images.contiguous()) if images.dtype == torch.uint8 else images.contiguous().float()
        self._check_batch(img)
        self.forward_generation += 1
        for l in range(self.arch.layers):
            self.block_generation[l] = self.block_generation.get(l, 0) + 1
        feat = torch.empty((B, self.arch.embed_dim), dtype=torch.float32, device=self.device)
        fn = self.lib.pevit_visual_forward_u8 if img.dtype == torch.uint8 else self.lib.pevit_visual_forward
        _lib.check(fn(self._ctx, _lib.stream_ptr(), _lib.ptr(img), _lib.ptr(feat), B, int(save)), "pevit_visual_forward")
        return feat

    def predict(self, images: torch.Tensor, logits_out=None, return_features: bool = False):
        """images -> logits in ONE engine call, for evaluation (``pevit_predict``): the tower in its inference form (nothing is
        stored for a backward pass), BatchNorm1d in eval mode on ``running_mean`` / ``running_var``, the Linear head.  Bit-identical
        to ``head_forward_backward(visual_forward(images, save=False), None, bn_training=False)[0]``; parameters, gradients,
        momentum and the running statistics are only read.  Returns the logits (B, C) as a device tensor without synchronising --
        ``logits_out``: a caller-owned f32 destination -- and ``(logits, features (B, D))`` with ``return_features``.  Like every
        forward it invalidates the activations a pending backward would read."""
        self.dp_flush()                # a pipelined DP step may still owe the parameter update
        B = images.shape[0]
        img = self._input(images.contiguous()) if images.dtype == torch.uint8 else images.contiguous().float()
        self._check_batch(img)
        self.forward_generation += 1
        for l in range(self.arch.layers):
            self.block_generation[l] = self.block_generation.get(l, 0) + 1
        if logits_out is None:
            logits = torch.empty((B, self.num_classes), dtype=torch.float32, device=self.device)
        else:
            logits = self._out_buf(logits_out, (B, self.num_classes))
        feat = torch.empty((B, self.arch.embed_dim), dtype=torch.float32, device=self.device) if return_features else None
        fn = self.lib.pevit_predict_u8 if img.dtype == torch.uint8 else self.lib.pevit_predict
        _lib.check(fn(self._ctx, _lib.stream_ptr(), _lib.ptr(img), _lib.ptr(self.running_mean), _lib.ptr(self.running_var),
                      _lib.ptr(logits), _lib.ptr(feat), B), "pevit_predict")
        return (logits, feat) if return_features else logits

    def _inference_walk(self, images):
        """What ``predict`` does before its engine call: flush a pipelined DP step, check the batch, bump the generations (the
        walk overwrites the activations a pending backward would read)."""
        self.dp_flush()
        img = self._input(images.contiguous()) if images.dtype == torch.uint8 else images.contiguous().float()
        self._check_batch(img)
        self.forward_generation += 1
        for l in range(self.arch.layers):
            self.block_generation[l] = self.block_generation.get(l, 0) + 1
        return img

    def encode_image(self, images: torch.Tensor) -> torch.Tensor:
        """images -> features (B, D) through the inference forms of the tower, without a head (``pevit_encode_image``;
        CLIP.encode_image for evaluation).  The bits ``predict(..., return_features=True)`` returns; nothing is stored for a
        backward pass; no synchronise."""
        img = self._inference_walk(images)
        B = img.shape[0]
        feat = torch.empty((B, self.arch.embed_dim), dtype=torch.float32, device=self.device)
        fn = self.lib.pevit_encode_image_u8 if img.dtype == torch.uint8 else self.lib.pevit_encode_image
        _lib.check(fn(self._ctx, _lib.stream_ptr(), _lib.ptr(img), _lib.ptr(feat), B), "pevit_encode_image")
        return feat

    def zeroshot(self, images: torch.Tensor, text_cd: torch.Tensor, scale: float = 100.0, probs_out=None,
                 return_logits: bool = False, return_features: bool = False):
        """images -> zero-shot class probabilities ``softmax(scale * normalize(features) @ text_cd.T)`` in ONE engine call
        (``pevit_zeroshot``): the inference walk, then the cosine head and its softmax in one exact-f32 launch.  ``text_cd``:
        contiguous f32 (C, D) on this device, CLASS-major, one unit vector per row -- the transpose of the reference's (D, C)
        text features; C is independent of ``num_classes``, 1 <= C <= 1024.  Returns the probabilities (B, C) as a device tensor
        without synchronising (``probs_out``: a caller-owned f32 destination), followed by the logits with ``return_logits``
        and the features (B, D) with ``return_features``.  Parameters, gradients and running statistics are only read."""
        D = self.arch.embed_dim
        if text_cd.device != self.device or text_cd.dtype != torch.float32 or not text_cd.is_contiguous() or text_cd.dim() != 2 \
                or text_cd.shape[1] != D:
            raise _lib.PevitError(f"text_cd must be a contiguous float32 tensor (C, {D}) on {self.device}; got "
                                  f"{tuple(text_cd.shape)} {text_cd.dtype} on {text_cd.device}")
        img = self._inference_walk(images)
        B, Cc = img.shape[0], text_cd.shape[0]
        if probs_out is None:
            probs = torch.empty((B, Cc), dtype=torch.float32, device=self.device)
        else:
            probs = self._out_buf(probs_out, (B, Cc))
        logits = torch.empty((B, Cc), dtype=torch.float32, device=self.device) if return_logits else None
        feat = torch.empty((B, D), dtype=torch.float32, device=self.device) if return_features else None
        fn = self.lib.pevit_zeroshot_u8 if img.dtype == torch.uint8 else self.lib.pevit_zeroshot
        _lib.check(fn(self._ctx, _lib.stream_ptr(), _lib.ptr(img), _lib.ptr(text_cd), Cc, float(scale), _lib.ptr(probs),
                      _lib.ptr(logits), _lib.ptr(feat), B), "pevit_zeroshot")
        out = (probs,) + ((logits,) if return_logits else ()) + ((feat,) if return_features else ())
        return out if len(out) > 1 else probs

    # ------------------------------------------------------------------ linear probe on cached features (csrc/probe.hip)
    def _check_cache(self, feats, index=None, labels=None):
        """What the probe entries read through raw pointers: a contiguous f32 (rows, D) feature matrix, int64 row indices, and
        labels indexed like the matrix -- int64 (rows,) or f32 (rows, num_classes) -- all on this engine's device.  Returns True for
        multi-label targets."""
        D = self.arch.embed_dim
        if feats.device != self.device or feats.dtype != torch.float32 or not feats.is_contiguous() or feats.dim() != 2 \
                or feats.shape[1] != D or feats.shape[0] < 1:
            raise _lib.PevitError(f"cached features must be a contiguous float32 tensor (rows, {D}) on {self.device}; got "
                                  f"{tuple(feats.shape)} {feats.dtype} on {feats.device}")
        if index is not None and (index.device != self.device or index.dtype != torch.int64 or not index.is_contiguous()
                                  or index.dim() != 1):
            raise _lib.PevitError(f"index must be a contiguous int64 vector on {self.device}; got {tuple(index.shape)} {index.dtype} "
                                  f"on {index.device}")
        if labels is None:
            return None
        return self._check_labels(labels, feats.shape[0])

    def probe_step(self, feats, index, labels, lr=0.0, momentum=0.9, weight_decay=0.0, nesterov=False, bn_training=True,
                   scale=1.0, update=True, logits_out=None, loss_out=None):
        """One training step of the linear probe on CACHED feature rows, two launches (``pevit_probe_step``): gather
        ``feats[index]``, BatchNorm1d, ``scale * Linear``, mean cross-entropy over ``labels[index]`` (int64 (rows,)) or BCE with
        logits over ``labels[index]`` (f32 (rows, C)), the head's gradients into ``self.grads`` and -- with ``update`` -- torch's
        SGD on the head.  ``update=False`` leaves parameters and momentum alone for ``optimizer_step(plan)``.  Only on a
        ``"none"`` engine.  Returns (logits, loss) as device tensors without synchronising."""
        self.dp_flush()
        # the matrix and its labels are the same tensors step after step: they are checked once, the index list every time
        # (keyed on everything _check_cache looks at: another tensor the allocator puts at the same address is checked again)
        seen = tuple((t.data_ptr(), tuple(t.shape), t.stride(), t.dtype, t.device) for t in (feats, labels))
        a = getattr(self, "_probe_args", None)
        if a is None or self._probe_seen != seen:
            bce = self._check_cache(feats, None, labels)
            a = self._probe_args = _lib.PevitProbeArgs()
            a.feat, a.rows = feats.data_ptr(), feats.shape[0]
            a.labels, a.targets = (None, labels.data_ptr()) if bce else (labels.data_ptr(), None)
            a.running_mean, a.running_var = self.running_mean.data_ptr(), self.running_var.data_ptr()
            self._probe_seen = seen
        if index.dtype != torch.int64 or index.device != self.device or index.dim() != 1 or not index.is_contiguous():
            raise _lib.PevitError(f"index must be a contiguous int64 vector on {self.device}; got {tuple(index.shape)} {index.dtype} "
                                  f"on {index.device}")
        B = index.shape[0]
        if update and self._optim_kind not in (None, "sgd"):
            raise _lib.PevitError(f"probe_step: the optimizer state belongs to {self._optim_kind!r}; call reset_optimizer() first")
        if not 2 <= B <= self.max_batch:
            raise _lib.PevitError(f"probe_step: batch {B} outside [2, {self.max_batch}] (max_batch of the bound workspace)")
        logits = self._logits[:B] if logits_out is None else self._out_buf(logits_out, (B, self.num_classes))
        loss = self._loss if loss_out is None else self._out_buf(loss_out, (1,))
        a.index, a.logits, a.loss = index.data_ptr(), logits.data_ptr(), loss.data_ptr()
        a.batch, a.bn_training, a.update = B, int(bn_training), int(update)
        a.flags = int(self._steps == 0) | (2 if nesterov else 0)
        a.scale, a.lr, a.momentum, a.weight_decay = float(scale), float(lr), float(momentum), float(weight_decay)
        _lib.check(self.lib.pevit_probe_step(self._ctx, _lib.stream_ptr(), C.byref(a)), "pevit_probe_step")
        if update:
            self._steps += 1
        return logits, loss

    def probe_predict(self, feats, index=None, first_row=0, count=None, scale=1.0, logits_out=None):
        """``scale * Linear(BatchNorm1d_eval(rows))`` over cached feature rows in ONE launch for any number of rows
        (``pevit_probe_predict``): ``feats[index]``, or ``feats[first_row:first_row + count]`` without an index.  A row's bits do
        not depend on the other rows of the call.  Parameters and running statistics are only read; no synchronise."""
        self.dp_flush()
        self._check_cache(feats, index)
        n = index.shape[0] if index is not None else (feats.shape[0] - first_row if count is None else count)
        if logits_out is None:
            logits = torch.empty((n, self.num_classes), dtype=torch.float32, device=self.device)
        else:
            logits = self._out_buf(logits_out, (n, self.num_classes))
        a = _lib.PevitProbePredictArgs()
        a.feat, a.rows = feats.data_ptr(), feats.shape[0]
        a.index_or_null = None if index is None else index.data_ptr()
        a.first_row, a.count = int(first_row), int(n)
        a.running_mean, a.running_var = self.running_mean.data_ptr(), self.running_var.data_ptr()
        a.scale, a.logits = float(scale), logits.data_ptr()
        _lib.check(self.lib.pevit_probe_predict(self._ctx, _lib.stream_ptr(), C.byref(a)), "pevit_probe_predict")
        return logits

    def visual_backward(self, dfeat: torch.Tensor):
        self.dp_flush()
        B = dfeat.shape[0]
        d = dfeat.contiguous().float()
        _lib.check(self.lib.pevit_visual_backward(self._ctx, _lib.stream_ptr(), _lib.ptr(d), B), "pevit_visual_backward")

    def head_forward_backward(self, feat, labels, bn_training=True, need_dfeat=True):
        """BatchNorm1d -> Linear -> loss, forward and backward.  ``labels``: int64 (B,) -> cross-entropy, float32 (B, num_classes)
        -> BCEWithLogitsLoss, None -> forward only."""
        self.dp_flush()
        B = feat.shape[0]
        fn = self.lib.pevit_head_forward_backward if labels is None else self._head_fn(labels, B)
        logits = torch.empty((B, self.num_classes), dtype=torch.float32, device=self.device)
        loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        dfeat = torch.empty_like(feat) if (need_dfeat and labels is not None) else None
        _lib.check(fn(
            self._ctx, _lib.stream_ptr(), _lib.ptr(feat.contiguous()), _lib.ptr(labels), _lib.ptr(self.running_mean),
            _lib.ptr(self.running_var), int(bn_training), _lib.ptr(logits), _lib.ptr(loss), _lib.ptr(dfeat), B),
            "pevit_head_forward_backward")
        return logits, loss, dfeat

    def zero_grad(self):
        self.dp_flush()
        _lib.check(self.lib.pevit_zero_grads(self._ctx, _lib.stream_ptr()), "pevit_zero_grads")

    def forward_backward(self, images, labels, bn_training=True, logits_out=None, loss_out=None):
        """zero_grad -> forward -> loss -> backward; gradients land in ``self.grads``.  ``labels``: int64 (B,) class indices
        (cross-entropy) or float32 (B, num_classes) multi-label targets (BCEWithLogitsLoss, mean over B * num_classes).  Returns
        (logits, loss) as device tensors without synchronising (the reference's
        ``loss.item()`` per step, kadaptation_clip.py:354, is the caller's choice).  ``logits_out`` (B, C) / ``loss_out`` (1,):
        caller-owned f32 destinations (an epoch buffer of the harness) instead of the engine's per-step buffers, which the
        next step overwrites."""
        B = images.shape[0]
        images = self._input(images)
        bce = self._check_batch(images, labels)
        self.forward_generation += 1
        logits = self._logits[:B] if logits_out is None else self._out_buf(logits_out, (B, self.num_classes))
        loss = self._loss if loss_out is None else self._out_buf(loss_out, (1,))
        fn = self._train_fn(images, bce)
        _lib.check(fn(self._ctx, _lib.stream_ptr(), _lib.ptr(images), _lib.ptr(labels), _lib.ptr(self.running_mean),
                      _lib.ptr(self.running_var), int(bn_training), _lib.ptr(logits), _lib.ptr(loss), B),
                   "pevit_train_forward_backward")
        return logits, loss

    def _out_buf(self, t, shape):
        if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
            raise _lib.PevitError(f"output buffer must be a contiguous float32 tensor {tuple(shape)} on {self.device}; got "
                                  f"{tuple(t.shape)} {t.dtype} on {t.device}")
        return t

    def sgd_step(self, lr, momentum=0.9, weight_decay=0.0, grad_scale=1.0, nesterov=False, _pipelined=False):
        if not _pipelined:             # a direct call while a pipelined update is still running on the second stream
            self.dp_flush()
        if self._optim_kind not in (None, "sgd"):
            raise _lib.PevitError(f"sgd_step: the optimizer state belongs to {self._optim_kind!r}; call reset_optimizer() first")
        flags = int(self._steps == 0) | (2 if nesterov else 0)
        _lib.check(self.lib.pevit_sgd_step(self._ctx, _lib.stream_ptr(), lr, momentum, weight_decay, grad_scale, flags),
                   "pevit_sgd_step")
        # the fused SGD kernel skips the update on device when a stream-K hand-off of this step timed out; the host reads
        # the error word on the first step and then every STREAMK_CHECK_EVERY steps (each check synchronises the stream)
        # ... and with the flat all-reduce as the exchange EVERY step: a rank whose reduction gave up withholds its update while its
        # peers apply theirs, and replicas must not drift apart for 64 steps before anybody notices
        if self._steps % self.STREAMK_CHECK_EVERY == 0 or getattr(self, "_flat_ar", None) is not None:
            self.check_streamk()
        self._steps += 1

    def _adam_state(self):
        """Adam's second moment, allocated (zero) on first use and made known to the context."""
        if self.exp_avg_sq is None:
            self.exp_avg_sq = torch.zeros_like(self.params)
            self._bind_optim_state()
        return self.exp_avg_sq

    def _bind_optim_state(self):
        if self._group_of is None:
            self._group_of = torch.full((self.n_params,), _lib.OPTIM_NO_GRAD, dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.pevit_set_optim_state(self._ctx, _lib.ptr(self.exp_avg_sq), _lib.ptr(self._group_of)),
                   "pevit_set_optim_state")

    def optimizer_step(self, plan: "OptimPlan", grad_scale=1.0, _pipelined=False):
        """``optimizer.step()`` of the optimizer ``plan`` describes (torch.optim.Adam / AdamW, or SGD whose groups differ) as one
        launch of the fused kernel (csrc/optim.hip) over the flat buffer.  ``exp_avg`` lives in ``self.momentum``, ``exp_avg_sq`` in
        ``self.exp_avg_sq``; the Adam step ``t`` is this engine's count of optimizer calls since ``reset_optimizer()`` (there is
        no device-side counter): an update that a raised error word withholds still counts, so after ``clear_streamk_error()``
        the bias corrections are those of the call count, one ahead of the updates applied, per withheld step.  The state belongs to one optimizer kind: a plan of another kind raises until
        ``reset_optimizer()``.  Error words, the periodic check and ``dp_flush()`` behave as in ``sgd_step``."""
        if not _pipelined:
            self.dp_flush()
        prior = self._optim_kind or ("sgd" if self._steps else None)
        if prior is not None and prior != plan.kind:
            raise _lib.PevitError(f"optimizer_step: the optimizer state belongs to {prior!r}, the plan is {plan.kind!r}; call "
                                  f"reset_optimizer() first")
        n = len(plan.groups)
        if not 1 <= n <= _lib.OPTIM_MAX_GROUPS:
            raise _lib.PevitError(f"optimizer_step: {n} parameter groups (1 to {_lib.OPTIM_MAX_GROUPS} are supported)")
        if plan.kind != "sgd":
            self._adam_state()
        host = plan.group_of
        seen = (host, host._version)            # the same tensor, not written since: nothing to compare
        if self._group_of_seen is None or seen[0] is not self._group_of_seen[0] or seen[1] != self._group_of_seen[1]:
            if host.dtype != torch.uint8 or host.numel() != self.n_params:
                raise _lib.PevitError(f"optimizer_step: group_of must hold {self.n_params} uint8 entries")
            if self._group_of_host is None or not torch.equal(host, self._group_of_host):      # membership changed: the one upload
                if self._group_of is None:
                    self._bind_optim_state()
                self._group_of.copy_(host)
                self._group_of_host = host.clone()
            self._group_of_seen = seen
        groups = (_lib.PevitOptimGroup * n)()
        for dst, g in zip(groups, plan.groups):
            dst.lr, dst.weight_decay, dst.momentum = g["lr"], g["weight_decay"], g.get("momentum", 0.0)
            dst.beta1, dst.beta2, dst.eps = g.get("beta1", 0.0), g.get("beta2", 0.0), g.get("eps", 0.0)
            dst.nesterov = int(bool(g.get("nesterov", False)))
        _lib.check(self.lib.pevit_optim_step(self._ctx, _lib.stream_ptr(), _lib.OPTIM_KINDS[plan.kind], groups, n,
                                             self._steps + 1, grad_scale, int(self._steps == 0)), "pevit_optim_step")
        self._optim_kind = plan.kind
        if self._steps % self.STREAMK_CHECK_EVERY == 0 or getattr(self, "_flat_ar", None) is not None:
            self.check_streamk()
        self._steps += 1

    def _update(self, optimizer, lr, momentum, weight_decay, grad_scale, nesterov, _pipelined=False):
        """The step's one dispatch point between the plain-SGD kernel and a planned optimizer."""
        if optimizer is not None:
            self.optimizer_step(optimizer, grad_scale, _pipelined=_pipelined)
        else:
            self.sgd_step(lr, momentum, weight_decay, grad_scale, nesterov, _pipelined=_pipelined)

    STREAMK_CHECK_EVERY = 64

    def check_streamk(self):
        """Stream-K GEMMs hand partial tiles between workgroups inside one launch; a consumer that never saw its
        producer gives up after ~1 s and raises an error word instead of hanging.  Fails loudly if that happened, and says how
        many optimizer updates the fused SGD kernel withheld since.  The word is NOT cleared here: every later update is
        withheld and every later check raises again until the caller acknowledges with ``clear_streamk_error()``."""
        word, skipped = C.c_uint(), C.c_uint()
        _lib.check(self.lib.pevit_streamk_status(self._ctx, _lib.stream_ptr(), C.byref(word), C.byref(skipped)), "pevit_streamk_status")
        if getattr(self, "_flat_ar", None) is not None:       # the DP exchange's error word (updates were withheld on device while raised)
            self._flat_ar.check(stream=self._flat_ar_stream)
        if word.value:
            raise _lib.PevitError(f"stream-K GEMM hand-off timed out: the logits / loss returned since are invalid and "
                                  f"{skipped.value} optimizer update(s) were withheld on device (parameters and momentum are those "
                                  f"of the last good step); call clear_streamk_error() to resume")

    def clear_streamk_error(self) -> bool:
        """Acknowledge a stream-K error (clears the device word and the withheld-update counter); True if one was pending."""
        rc = self.lib.pevit_streamk_error(self._ctx, _lib.stream_ptr())
        if rc < 0:
            raise _lib.PevitError("pevit_streamk_error failed")
        return rc > 0

    PROF_KINDS = {0: "ln_fwd", 1: "ln_bwd", 2: "attn_fwd", 3: "attn_bwd", 4: "delta_add", 5: "lowrank_u", 6: "lowrank_grad",
                  7: "im2col", 8: "lowrank_bwd", 9: "attn_fwd_delta", 10: "adapter_fwd", 11: "adapter_bwd"}     # include/pevit_hip.h: enum pevit_prof_kind

    def profile_gemms(self, fn, max_launches=8192, all_kernels=False):
        """Run ``fn()`` with HIP events around every GEMM launch; returns (ms, flops, launches) of the GEMM family; the
        algorithmic operand+result bytes of those launches are left in ``self.last_profile_bytes``, the per-shape table in
        ``self.last_profile_by_shape``.  ``all_kernels``: the HBM-bound kernels of the step are bracketed too and land in
        ``self.last_profile_hbm`` = {kernel: [launches, ms, algorithmic bytes]}."""
        self.tune("profile_all", int(all_kernels))
        try:
            _lib.check(self.lib.pevit_profile_begin(self._ctx, max_launches), "pevit_profile_begin")
            fn()
            ms, fl, by, n = C.c_double(), C.c_double(), C.c_double(), C.c_int()
            _lib.check(self.lib.pevit_profile_end(self._ctx, C.byref(ms), C.byref(fl), C.byref(by), C.byref(n)),
                       "pevit_profile_end")
        finally:
            self.tune("profile_all", 0)
        self.last_profile_bytes = by.value
        # per launch: (epilogue, M, N, K) -> [launches, ms, flops, bytes]
        per, hbm, n_gemm = {}, {}, 0
        one_ms, one_fl, one_by, shape = C.c_double(), C.c_double(), C.c_double(), (C.c_int * 4)()
        for i in range(n.value):
            _lib.check(self.lib.pevit_profile_launch(self._ctx, i, C.byref(one_ms), C.byref(one_fl), shape), "pevit_profile_launch")
            _lib.check(self.lib.pevit_profile_launch_bytes(self._ctx, i, C.byref(one_by)), "pevit_profile_launch_bytes")
            if shape[0] >= 100:
                e = hbm.setdefault(self.PROF_KINDS.get(shape[0] - 100, str(shape[0] - 100)), [0, 0.0, 0.0])
                e[0] += 1; e[1] += one_ms.value; e[2] += one_by.value
            else:
                n_gemm += 1
                e = per.setdefault(tuple(shape), [0, 0.0, 0.0, 0.0])
                e[0] += 1; e[1] += one_ms.value; e[2] += one_fl.value; e[3] += one_by.value
        self.last_profile_by_shape = per
        self.last_profile_hbm = hbm
        return ms.value, fl.value, n_gemm

    def reset_optimizer(self):
        self.dp_flush()
        self._steps = 0
        self._optim_kind = None
        self.momentum.zero_()
        if self.exp_avg_sq is not None:
            self.exp_avg_sq.zero_()

    def reset_run(self):
        """State a fresh ``Classifier`` would have, with the frozen backbone left resident (the
        reference rebuilds everything for each of its ~90 sweep runs).  Clears both optimizer moments."""
        self.dp_flush()
        self.reset_optimizer()
        self.params.zero_(); self.grads.zero_()
        self.running_mean.zero_(); self.running_var.fill_(1.0)

    def train_step(self, images, labels, lr=None, momentum=0.9, weight_decay=0.0, bn_training=True, process_group=None,
                   world_size=1, nesterov=False, logits_out=None, loss_out=None, optimizer=None):
        """One reference ``train_one`` iteration (kadaptation_clip.py:347-353).  With DP the flat gradient buffer
        is the only thing that crosses xGMI (the frozen backbone never does); how it is exchanged is ``dp_exchange_mode``
        (default: one in-stream all-reduce behind the fused forward/backward call, 1/world folded into the SGD kernel).
        ``optimizer``: an ``OptimPlan`` (Adam, AdamW, SGD with several groups) -- the update is then ``optimizer_step(plan)``
        wherever it is ``sgd_step`` otherwise, and ``lr`` / ``momentum`` / ``weight_decay`` / ``nesterov`` are not read."""
        if optimizer is None and lr is None:
            raise TypeError("train_step: lr (plain SGD) or optimizer (an OptimPlan) is required")
        if world_size <= 1:
            logits, loss = self.forward_backward(images, labels, bn_training, logits_out, loss_out)
            self._update(optimizer, lr, momentum, weight_decay, 1.0, nesterov)
            return logits, loss
        if self.dp_exchange_mode == "pipelined":
            return self._train_step_pipelined(images, labels, lr, momentum, weight_decay, bn_training, process_group, world_size,
                                              nesterov, logits_out, loss_out, optimizer)
        logits, loss = self.forward_backward_dp(images, labels, bn_training, process_group)
        if logits_out is not None:
            logits_out.copy_(logits)
        if loss_out is not None:
            loss_out.copy_(loss)
        self._update(optimizer, lr, momentum, weight_decay, 1.0 / world_size, nesterov)
        return logits, loss

    # ---- DP with the exchange under the next step's stem (round 5) ----------------------------------------------------------------
    def _train_step_pipelined(self, images, labels, lr, momentum, weight_decay, bn_training, process_group, world_size, nesterov,
                              logits_out, loss_out, optimizer=None):
        """``dp_exchange_mode = "pipelined"``: the fused forward/backward call on the current stream; the all-reduce of the flat
        gradient buffer and the fused SGD kernel on a SECOND stream behind it; the next fused call runs its stem (patch gather,
        patch embedding, ln_pre: ~70 us that read no trainable parameter) and only then waits, on the device, for the update
        (``pevit_set_step_gate``).  The exchange's latency and the cross-stream hand-overs around the collective leave the critical
        path.  Same kernels, same order of arithmetic as the other modes: bit-identical results (tests/test_gpu_dp.py).
        The caller's obligations: every step of a run goes through ``train_step`` on ONE stream; ``dp_flush()`` before anything
        else reads parameters / momentum / gradients or launches on them (validation, ``state_dict``, another mode) -- the
        engine's own entry points that do so call it."""
        cur = torch.cuda.current_stream(self.device)
        st = getattr(self, "_pipe", None)
        if st is None:
            st = self._pipe = {"stream": torch.cuda.Stream(self.device), "grads": torch.cuda.Event(), "params": torch.cuda.Event(),
                               "open": False}
            st["params"].record(cur)                       # (creates the event: nothing to wait for before the first step)
            _lib.check(self.lib.pevit_set_step_gate(self._ctx, C.c_void_p(st["params"].cuda_event)), "pevit_set_step_gate")
        st["open"] = True
        logits, loss = self.forward_backward(images, labels, bn_training, logits_out, loss_out)     # waits for st["params"] behind its stem
        st["grads"].record(cur)
        with torch.cuda.stream(st["stream"]):
            st["stream"].wait_event(st["grads"])
            xt = self._xt_pair()
            if xt: xt[0].record(st["stream"])
            self._exchange(self.grads, process_group, in_stream=True).wait()
            if xt: xt[1].record(st["stream"])
            self._update(optimizer, lr, momentum, weight_decay, 1.0 / world_size, nesterov, _pipelined=True)
            st["params"].record(st["stream"])
        return logits, loss

    # ---- how long the exchange takes on the device (bench.py N > 1: `exchange_us_per_step`) ---------------------------------------
    def time_exchange(self, on: bool = True):
        """Bracket every gradient exchange of the DP step with a pair of events on the stream it is enqueued on (single / staged:
        the compute stream -- for staged the pair brackets the WAITS at the end of the backward, i.e. the part of the three
        asynchronous all-reduces that the backward did not hide; pipelined: the second stream).  ``exchange_times_us()`` reads
        them back."""
        self._xt = [] if on else None

    def _xt_pair(self):
        if getattr(self, "_xt", None) is None:
            return None
        pair = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        self._xt.append(pair)
        return pair

    def exchange_times_us(self):
        """Microseconds of every bracketed exchange since time_exchange(True) (synchronises the device)."""
        torch.cuda.synchronize(self.device)
        return [a.elapsed_time(b) * 1e3 for a, b in (getattr(self, "_xt", None) or [])]

    def dp_flush(self):
        """Pipelined DP: make the current stream wait for the last exchange + update (no-op otherwise)."""
        st = getattr(self, "_pipe", None)
        if st is not None and st["open"]:
            torch.cuda.current_stream(self.device).wait_event(st["params"])
            st["open"] = False

    def dp_pipeline_off(self):
        """Leave the pipelined schedule: flush, detach the step gate from the context, drop the second stream."""
        self.dp_flush()
        if getattr(self, "_pipe", None) is not None:
            _lib.check(self.lib.pevit_set_step_gate(self._ctx, None), "pevit_set_step_gate")
            self._pipe = None

    # ---- whole-step HIP graph -----------------------------------------------------
    def capture_train_step(self, images, labels, lr=None, momentum=0.9, weight_decay=0.0, bn_training=True, nesterov=False,
                           optimizer=None):
        """Capture ``forward_backward + sgd_step`` on THESE buffers (pointers, batch, hyper-parameters and BatchNorm mode are baked
        in) into a HIP graph and return a callable that replays it: one hipGraphLaunch instead of ~200 kernel launches from the
        C call.  The step counter, the periodic error-word check and the results (``self._logits``, ``self._loss``) behave as in
        ``train_step``.  At least one eager step must have run (the first SGD step has no momentum buffer to read, and the
        library's one-time attribute calls are not stream operations).  Same kernels, same order: bit-identical to eager
        (tests/test_gpu_mirror.py::test_graph_replay_equals_eager).  Measured: profiles/r05_graph_capture.md.
        Plain SGD only: the Adam step count ``t`` is kept by the host and reaches the kernel by value, so a captured launch would
        replay one fixed ``t``; an ``optimizer`` plan (``optimizer_step``) raises here until a device-side counter exists."""
        if optimizer is not None:
            raise _lib.PevitError("capture_train_step captures the plain-SGD step only: the planned optimizers (Adam, AdamW, "
                                  "per-group SGD) take their step count and hyper-parameters by value on every launch")
        if lr is None:
            raise TypeError("capture_train_step: lr is required")
        if self._steps == 0:
            raise _lib.PevitError("capture_train_step: run one eager train_step first (first-step flag, one-time kernel attributes)")
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise _lib.PevitError("capture_train_step is a single-GPU tool: the captured step has no gradient exchange")
        # leaves the pipelined schedule altogether: a step gate still attached to the context would bake a wait on an event
        # recorded OUTSIDE the capture (and the gated zero_grads path) into the graph
        self.dp_pipeline_off()
        B = images.shape[0]
        if self._needs_resize(images):
            raise _lib.PevitError("capture_train_step: the batch needs the input resize, which is not part of the captured step: "
                                  "capture on resize_u8(images) copied to a buffer of your own")
        fn = self._train_fn(images, self._check_batch(images, labels))
        flags = 2 if nesterov else 0
        logits, loss = self._logits[:B], self._loss
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
                _lib.check(fn(self._ctx, _lib.stream_ptr(), _lib.ptr(images), _lib.ptr(labels), _lib.ptr(self.running_mean),
                              _lib.ptr(self.running_var), int(bn_training), _lib.ptr(logits), _lib.ptr(loss), B),
                           "pevit_train_forward_backward (capture)")
                _lib.check(self.lib.pevit_sgd_step(self._ctx, _lib.stream_ptr(), lr, momentum, weight_decay, 1.0, flags),
                           "pevit_sgd_step (capture)")
        torch.cuda.current_stream(self.device).wait_stream(side)
        keep = (images, labels)                     # the graph reads these addresses on every replay

        def replay():
            self.forward_generation += 1
            graph.replay()
            if self._steps % self.STREAMK_CHECK_EVERY == 0:
                self.check_streamk()
            self._steps += 1
            return logits, loss
        replay.graph, replay.buffers = graph, keep
        return replay

    def use_flat_allreduce(self, process_group=None):
        """Exchange the gradient buckets with pevit_allreduce_flat (dp.FlatAllReduce: IPC-mapped peer mailboxes, copy-engine
        pushes, deterministic local reduction on a side stream) instead of the process group's all-reduce."""
        from . import dp
        self._flat_ar = dp.FlatAllReduce(self.n_params, group=process_group, device=self.device)
        self._flat_ar_stream = torch.cuda.Stream(self.device)
        # a bucket whose exchange gave up (a peer never arrived, sizes disagree) must not reach the parameters: the fused SGD
        # kernel reads the all-reduce's error word next to the stream-K one and withholds the update while either is raised
        _lib.check(self.lib.pevit_set_external_poison(self._ctx, C.c_void_p(self._flat_ar.error_word())), "pevit_set_external_poison")
        return self._flat_ar

    def _exchange(self, view, process_group, in_stream=False):
        """Start the sum all-reduce of one gradient bucket; returns something with .wait().
        in_stream: nothing is to run beside the exchange (the single-exchange schedule): the SYNCHRONOUS form of the collective,
        which this torch enqueues on the CURRENT stream.  Measured on a 1-rank RCCL group (scripts/r5_dp_hosttime.py): a round trip
        through a second stream -- what ``async_op=True`` + ``wait()`` is, with or without a collective on it -- costs 74 us of
        device time per step on this platform, the synchronous call 7 us."""
        import torch.distributed as dist
        ar = getattr(self, "_flat_ar", None)
        if ar is None and in_stream:
            dist.all_reduce(view, op=dist.ReduceOp.SUM, group=process_group)

            class _Done:
                def wait(_self):
                    pass
            return _Done()
        if ar is None:
            return dist.all_reduce(view, op=dist.ReduceOp.SUM, group=process_group, async_op=True)
        if in_stream:
            ar.all_reduce(view, stream=torch.cuda.current_stream(self.device))

            class _Done2:
                def wait(_self):
                    pass
            return _Done2()
        cur, side = torch.cuda.current_stream(self.device), self._flat_ar_stream
        ready = torch.cuda.Event(); ready.record(cur)
        side.wait_event(ready)                          # the bucket's gradients are final
        ar.all_reduce(view, stream=side)
        done = torch.cuda.Event(); done.record(side)

        class _W:
            def wait(_self):
                torch.cuda.current_stream(self.device).wait_event(done)
        return _W()

    #: how the DP step exchanges the gradients: "single" = the fused forward/backward call, then ONE all-reduce of the whole
    #: flat buffer (406 KB for KAdaptation) | "staged" = the backward cut into stages with three overlapped buckets (rounds 2-4) |
    #: "pipelined" (train_step only) = "single" with the exchange + SGD on a second stream under the NEXT step's stem.
    #: Round 5 made "single" the default: the exchange is latency-bound at this size, so what the staged route can hide is the
    #: transfer of two of its three buckets, while the LAST bucket's latency is exposed either way -- and the staging itself (a
    #: second reduce / chain / rule-sum group, three round trips through the collective's stream at ~74 us each, stream-K off)
    #: costs 3.6 % of the step on one rank against 0.2 % for one in-stream exchange behind the fused call
    #: (bench.py --dp-route; profiles/r05_dp_single_exchange.md).
    dp_exchange_mode = "single"

    def forward_backward_dp(self, images, labels, bn_training=True, process_group=None, mode=None):
        """forward_backward() followed by the gradient exchange; leaves the SUM over ranks in ``self.grads``.
        mode "single" (default, ``dp_exchange_mode``): the fused call, then one all-reduce of the flat gradient buffer.
        mode "staged": the call cut into stages so that the exchange overlaps the backward -- three buckets of the flat buffer, each
        all-reduced asynchronously as soon as its gradients are final:  head (after the head backward) | blocks L/2..L-1 (after
        the upper half of the tower backward) | shared rules + blocks 0..L/2-1 (at the end).  Same kernels in the same order as
        the fused call either way, so a single rank reproduces forward_backward() bit for bit."""
        mode = mode or self.dp_exchange_mode
        self.dp_flush()
        if mode == "pipelined":
            raise ValueError("forward_backward_dp: the pipelined schedule spans the optimizer step -- use train_step")
        if mode == "single":
            if getattr(self, "_dp_streamk_off", False):        # (a staged step before this one switched it off)
                self.tune("gemm_streamk", 1); self._dp_streamk_off = False
            logits, loss = self.forward_backward(images, labels, bn_training)
            xt = self._xt_pair()
            if xt: xt[0].record()
            self._exchange(self.grads, process_group, in_stream=True).wait()
            if xt: xt[1].record()
            return logits, loss
        if mode != "staged":
            raise ValueError(f"forward_backward_dp: unknown mode {mode!r}")
        import torch.distributed as dist
        B = images.shape[0]
        images = self._input(images)
        self._check_batch(images, labels)
        if not getattr(self, "_dp_streamk_off", False):
            # the RCCL kernels of the overlapped all-reduce share the CUs with the second half of the backward: stream-K's
            # hand-off assumes all its workgroups are co-resident, so under DP the plain tilings are used instead
            self.tune("gemm_streamk", 0)
            self._dp_streamk_off = True
        self.zero_grad()
        feat = self.visual_forward(images, save=True)
        _lib.check(self._head_fn(labels, B)(
            self._ctx, _lib.stream_ptr(), _lib.ptr(feat), _lib.ptr(labels), _lib.ptr(self.running_mean),
            _lib.ptr(self.running_var), int(bn_training), _lib.ptr(self._logits), _lib.ptr(self._loss),
            _lib.ptr(self._dfeat(B)), B), "pevit_head_forward_backward")
        L = self.arch.layers
        mid = L // 2
        cut = self.lib.pevit_param_layer_offset(self._ctx, mid)
        work = [self._exchange(self.grads[self.n_tower:], process_group)]
        if self.n_tower == 0:                                  # frozen tower (linear probe): nothing below the head trains
            work[0].wait()
            return self._logits[:B], self._loss
        dfeat = self._dfeat(B)
        if mid > 0:
            _lib.check(self.lib.pevit_visual_backward_part(self._ctx, _lib.stream_ptr(), _lib.ptr(dfeat), B, L, mid),
                       "pevit_visual_backward_part")
            work.append(self._exchange(self.grads[cut:self.n_tower], process_group))
            _lib.check(self.lib.pevit_visual_backward_part(self._ctx, _lib.stream_ptr(), None, B, mid, 0),
                       "pevit_visual_backward_part")
            work.append(self._exchange(self.grads[:cut], process_group))
        else:
            self.visual_backward(dfeat)
            work.append(self._exchange(self.grads[:self.n_tower], process_group))
        xt = self._xt_pair()
        if xt: xt[0].record()
        for w in work:
            w.wait()
        if xt: xt[1].record()
        return self._logits[:B], self._loss

    def sync_replicas(self, process_group=None, src: int = 0):
        """Make every rank's trainable state identical to rank ``src``'s (parameters, momentum / exp_avg, exp_avg_sq, BatchNorm
        running statistics, step counter semantics): call once after the engines have been loaded and before the first DP step.
        ``exp_avg_sq`` travels only where it exists, that is after the first Adam / AdamW step, which every rank takes together;
        before it the buffer is unallocated on all of them and starts from zero, so a plain-SGD run allocates and sends nothing more
        than it did."""
        self.dp_flush()
        import torch.distributed as dist
        state = [self.params, self.momentum, self.running_mean, self.running_var]
        if self.exp_avg_sq is not None:
            state.append(self.exp_avg_sq)
        for t in state:
            dist.broadcast(t, src=src, group=process_group)

    def average_bn_buffers(self, process_group=None):
        """BatchNorm running statistics follow the LOCAL shards; average them across ranks before validation or a
        checkpoint (dp.average_bn_buffers)."""
        self.dp_flush()
        dp.average_bn_buffers(self.running_mean, self.running_var, process_group)

    def _dfeat(self, B):
        if getattr(self, "_dfeat_buf", None) is None or self._dfeat_buf.shape[0] < B:
            self._dfeat_buf = torch.empty((max(B, self.max_batch), self.arch.embed_dim), dtype=torch.float32, device=self.device)
        return self._dfeat_buf[:B]
