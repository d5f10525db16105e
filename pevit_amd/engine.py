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

from . import _lib
from ._context import EngineContext
from .engine_dp import DpMixin
from .engine_input import InputMixin
from .engine_optim import OptimMixin
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


class HipEngine(EngineContext, InputMixin, OptimMixin, DpMixin):
    """The context, the flat parameter buffer, weight loading and the forward / backward / inference / probe seams; the uint8
    input path (engine_input.py), the updates and error words (engine_optim.py) and the DP schedules (engine_dp.py) are mixins
    that keep no ``__init__`` of their own: ALL state of the engine is declared here."""

    def __init__(self, arch: VitArch, method: str, num_classes: int, max_batch: int, lora_rank: int = 4,
                 device: str | torch.device = "cuda:0", weight_format: str = "bf16"):
        super().__init__(device)
        self.arch, self.method, self.num_classes, self.lora_rank, self.max_batch = arch, method, num_classes, lora_rank, max_batch
        if weight_format not in _lib.WEIGHT_FORMATS:
            raise ValueError(f"weight_format {weight_format!r}: expected one of {sorted(_lib.WEIGHT_FORMATS)}")
        self.weight_format = weight_format
        dims = _lib.PevitDims(arch.width, arch.layers, arch.patch, arch.resolution, arch.embed_dim,
                              _lib.METHOD_IDS[method], lora_rank, num_classes, _lib.WEIGHT_FORMATS[weight_format])
        self._create("pevit_ctx_create", dims, max_batch)
        self.n_tower, self.n_params = self.lib.pevit_num_tower_params(self._ctx), self.lib.pevit_num_params(self._ctx)
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
        self.forward_generation = 0      # bumped by EVERY forward: each one overwrites the single activation workspace
        self.block_generation = {}       # per block: bumped by every forward THROUGH that block (blocks keep their own activations)
        self.attention_generation = {}   # per block: the block_generation its last attention_forward left (attention seam)
        self._logits = torch.empty((max_batch, num_classes), dtype=torch.float32, device=self.device)
        self._loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._probe_args = self._probe_seen = None       # probe_step: the arguments of the cached matrix last checked, and its identity
        self.last_profile_bytes = self.last_profile_by_shape = self.last_profile_hbm = None     # profile_gemms
        # ---- engine_input.py
        self._input_norm = None          # (mean, std) once set_input_normalization has run: uint8 batches are taken from then on
        self._input_resize, self._resize_center_crop = False, True       # set_input_resize(on, center_crop)
        self._resize_buf, self._resize_cache = None, {}  # resize_u8: its staging (on first use), (h, w, crop) -> device tables
        # ---- engine_optim.py
        self._steps = 0
        self.exp_avg_sq = None           # Adam / AdamW second moment: allocated on first use (optimizer_step); exp_avg is self.momentum
        # device copy of the last OptimPlan.group_of, a host copy of what was uploaded, and the (tensor, version) last compared with
        # it: an in-place edit of a plan is seen
        self._group_of = self._group_of_host = self._group_of_seen = None
        self._optim_kind = None          # which optimizer the momentum / exp_avg_sq buffers belong to (None: fresh, or plain sgd_step)
        # clip_grad_norm: {norm before clipping, clip coefficient, arrival count, -, one partial per workgroup}; zeroed once, here
        self._clip_scratch = torch.zeros(self.lib.pevit_clip_scratch_floats(self.n_params), dtype=torch.float32, device=self.device)
        self.last_grad_norm = self._clip_scratch[0]      # 0-dim device view: the norm the last clip found, never synchronised here
        self.max_grad_norm = None        # a bound: every update of train_step / a captured step clips the gradients to it first (None: off)
        # ---- engine_dp.py
        self._pipe = None                # the pipelined schedule's second stream, its two events and "open": an update is owed
        self._xt = None                  # time_exchange: the event pairs around every exchange (None: off)
        self._flat_ar = self._flat_ar_stream = None      # use_flat_allreduce: the dp.FlatAllReduce in the collective's place, its side stream
        self._dp_streamk_off = False     # a staged step switched the stream-K tilings off
        self._dfeat_buf = None           # staged schedule: the head's feature gradient between its two C calls

    def tune(self, key: str, value: int) -> int:
        """A/B-measurement knob of THIS context (include/pevit_hip.h: pevit_tune)."""
        return self.lib.pevit_tune(self._ctx, key.encode(), int(value))

    def ensure_batch(self, batch: int):
        """Grow the activation workspace so that steps of ``batch`` images fit (re-binds; weights stay)."""
        if batch <= self.max_batch:
            return
        torch.cuda.synchronize(self.device)
        self._bind(batch)
        self._logits = torch.empty((batch, self.num_classes), dtype=torch.float32, device=self.device)
        self._resize_buf = None          # the staging of resize_u8 follows the batch bound: allocated again on its next use
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
        return self.param_views(self.grads)

    # ------------------------------------------------------------------ frozen weights
    def load_state_dict(self, sd, prefix: str = "visual."):
        """Frozen backbone from an OpenAI-layout state-dict (any float dtype, any device)."""
        self.dp_flush()
        keep = self._load_blocks(sd, prefix, self.arch.layers)
        ts = [self._dev(sd[prefix + k]) for k in ("conv1.weight", "class_embedding", "positional_embedding", "ln_pre.weight",
                                                  "ln_pre.bias", "ln_post.weight", "ln_post.bias", "proj")]
        keep.append(ts)
        _lib.check(self.lib.pevit_load_stem(self._ctx, _lib.stream_ptr(), *[_lib.ptr(t) for t in ts]), "pevit_load_stem")
        if self.method == "compacter":
            self.load_phm_rule(sd[prefix + "transformer.phm_rule"])
        torch.cuda.current_stream().synchronize()     # the temporaries above may now be freed
        del keep
        self.load_trainable(sd)

    def load_phm_rule(self, rule: torch.Tensor):
        """Compacter's shared, frozen (4,4,4) rule (compacter_model.py:511-519) into the arena."""
        r = self._dev(rule)
        _lib.check(self.lib.pevit_load_phm_rule(self._ctx, _lib.stream_ptr(), _lib.ptr(r)), "pevit_load_phm_rule")
        torch.cuda.current_stream().synchronize()

    def load_trainable(self, sd):
        """Adapter / head tensors present in ``sd`` overlay the current values (model.py:1247-1250)."""
        with torch.no_grad():
            for name, v in self.param_views().items():
                if name in sd:
                    v.copy_(sd[name].to(device=self.device, dtype=torch.float32).view_as(v))

    # ------------------------------------------------------------------ what the C ABI's raw pointers may read
    def _check_bound(self, B):
        if B > self.max_batch:
            raise _lib.PevitError(f"batch {B} exceeds the bound workspace ({self.max_batch}): call ensure_batch")

    def _check_batch(self, images, labels=None):
        """f32 NCHW images -- or uint8 pixels once set_input_normalization has been called -- and int64 class indices (B,) or f32
        multi-label targets (B, num_classes), contiguous, on this engine's device.  Returns ``_check_labels``'s answer."""
        R = self.arch.resolution
        u8 = images.dtype == torch.uint8 and self._input_norm is not None
        if not self._fits(images, torch.uint8 if u8 else torch.float32, (None, 3, R, R)):
            self._refuse(images, f"images must be a contiguous float32 tensor (B,3,{R},{R})", " (or uint8 after set_input_normalization)")
        self._check_bound(images.shape[0])
        return None if labels is None else self._check_labels(labels, images.shape[0])

    def _check_labels(self, labels, B):
        """True for multi-label targets (BCEWithLogitsLoss), False for class indices (cross-entropy)."""
        if self._fits(labels, torch.int64, (B,)):
            return False
        if not self._fits(labels, torch.float32, (B, self.num_classes)):
            self._refuse(labels, f"labels must be a contiguous int64 tensor ({B},) or float32 tensor ({B}, {self.num_classes})")
        return True

    def _check_index(self, index):
        if not self._fits(index, torch.int64, (None,)):
            self._refuse(index, "index must be a contiguous int64 vector")

    def _check_cache(self, feats, index=None, labels=None):
        """What the probe entries read: a contiguous f32 (rows, D) feature matrix, int64 row indices, and labels indexed like the
        matrix -- int64 (rows,) or f32 (rows, num_classes) -- all on this engine's device.  Returns True for multi-label targets."""
        D = self.arch.embed_dim
        if not self._fits(feats, torch.float32, (None, D)) or feats.shape[0] < 1:
            self._refuse(feats, f"cached features must be a contiguous float32 tensor (rows, {D})")
        if index is not None:
            self._check_index(index)
        return None if labels is None else self._check_labels(labels, feats.shape[0])

    def _out_buf(self, t, shape):
        if not self._fits(t, torch.float32, tuple(shape)):
            self._refuse(t, f"output buffer must be a contiguous float32 tensor {tuple(shape)}")
        return t

    def _empty(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.device)

    def _out_or_new(self, t, shape):
        return self._empty(*shape) if t is None else self._out_buf(t, shape)

    def _step_out(self, B, logits_out, loss_out):       # caller-owned destinations, or the engine's per-step buffers
        return (self._logits[:B] if logits_out is None else self._out_buf(logits_out, (B, self.num_classes)),
                self._loss if loss_out is None else self._out_buf(loss_out, (1,)))

    def _train_fn(self, images, bce):
        """The fused C entry for this input form: uint8 or f32 pixels x cross-entropy or BCE."""
        return self._entry("pevit_train_forward_backward_bce" if bce else "pevit_train_forward_backward", images)

    def _entry(self, name, images):
        """The C entry ``name`` in the form that reads these pixels: ``name_u8`` for uint8, ``name`` for f32."""
        return getattr(self.lib, name + "_u8" if images.dtype == torch.uint8 else name)

    def _head_fn(self, labels, B):
        return self.lib.pevit_head_forward_backward_bce if self._check_labels(labels, B) else self.lib.pevit_head_forward_backward

    # ------------------------------------------------------------------ the seams of the tower, on (N,B,E) activations
    def _begin_forward(self, blocks, flush=True, attention=False):
        """Every forward starts here: a pipelined DP step may still owe the parameter update (``flush``; the fused step waits on
        the device instead); the forward overwrites the activation workspace and the saved slots of ``blocks``, so whatever a
        pending backward would read there is stale from now on.  ``attention``: the slots are left in the attention seam's form."""
        if flush:
            self.dp_flush()
        self.forward_generation += 1
        for l in blocks:
            self.block_generation[l] = self.block_generation.get(l, 0) + 1
            if attention:
                self.attention_generation[l] = self.block_generation[l]

    def _seam_forward(self, x_nbe, who, blocks, attention=False):
        """A forward seam's start: the (N,B,E) check, ``_begin_forward(blocks)``, then (f32 x, y like it, B)."""
        N, B, E = x_nbe.shape
        if (N, E) != (self.arch.tokens, self.arch.width) or x_nbe.device != self.device:
            raise _lib.PevitError(f"{who} expects ({self.arch.tokens}, B, {self.arch.width}) on {self.device}, "
                                  f"got {tuple(x_nbe.shape)} on {x_nbe.device}")
        self._begin_forward(blocks, attention=attention)
        x = x_nbe.contiguous().float()
        return x, torch.empty_like(x), B

    def _dy_dx(self, dy_nbe, need_dx):
        """A backward seam's operands: (f32 dy, dx like it or None, B)."""
        self.dp_flush()
        dy = dy_nbe.contiguous().float()
        return dy, (torch.empty_like(dy) if need_dx else None), dy_nbe.shape[1]

    def transformer_forward(self, x_nbe: torch.Tensor, save: bool = True) -> torch.Tensor:
        x, y, B = self._seam_forward(x_nbe, "transformer_forward", range(self.arch.layers))
        _lib.check(self.lib.pevit_transformer_forward(self._ctx, _lib.stream_ptr(), _lib.ptr(x), _lib.ptr(y), B, int(save)),
                   "pevit_transformer_forward")
        return y

    def blocks_forward(self, x_nbe: torch.Tensor, l_lo: int, l_hi: int, save: bool = True) -> torch.Tensor:
        """Blocks [l_lo, l_hi) on (N,B,E) activations (the reference's ResidualAttentionBlock.forward for one block)."""
        # every forward -- also one through a few blocks -- overwrites activations a pending whole-tower backward would read;
        # the output of block l_hi - 1 also lands in the saved INPUT of block l_hi
        x, y, B = self._seam_forward(x_nbe, "blocks_forward", range(l_lo, min(l_hi + 1, self.arch.layers)))
        _lib.check(self.lib.pevit_blocks_forward(self._ctx, _lib.stream_ptr(), _lib.ptr(x), _lib.ptr(y), B, int(save), l_lo, l_hi),
                   "pevit_blocks_forward")
        return y

    def blocks_backward(self, dy_nbe: torch.Tensor, l_lo: int, l_hi: int, need_dx: bool = True):
        dy, dx, B = self._dy_dx(dy_nbe, need_dx)
        _lib.check(self.lib.pevit_blocks_backward(self._ctx, _lib.stream_ptr(), _lib.ptr(dy), _lib.ptr(dx), B, l_lo, l_hi), "pevit_blocks_backward")
        return dx

    def attention_forward(self, x_nbe: torch.Tensor, layer: int, save: bool = True, weights: str | None = None):
        """MultiheadAttention.forward(x, x, x) of block ``layer`` (the reference's resblocks[layer].attn, model.py:837-944) on the
        attention INPUT x (N,B,E): returns (out_proj output without the residual, weights or None).  ``weights``: None
        (need_weights=False), "mean" ((B,N,N) head average) or "heads" ((B,H,N,N))."""
        if not 0 <= layer < self.arch.layers:
            raise _lib.PevitError(f"attention_forward: layer {layer} outside [0, {self.arch.layers})")
        if weights not in (None, "mean", "heads"):
            raise ValueError(f"weights={weights!r}: expected None, 'mean' or 'heads'")
        # the seam's activations live in the layer's saved slots: a pending backward through the tower or through this block is
        # no longer possible
        (x, y, B), N = self._seam_forward(x_nbe, "attention_forward", (layer,), attention=True), self.arch.tokens
        w = None if weights is None else self._empty(B, N, N) if weights == "mean" else self._empty(B, self.arch.heads, N, N)
        _lib.check(self.lib.pevit_attention_forward(self._ctx, _lib.stream_ptr(), layer, _lib.ptr(x), _lib.ptr(y), B, int(save),
                                                    _lib.ptr(w), int(weights != "heads")), "pevit_attention_forward")
        return y, w

    def attention_backward(self, dy_nbe: torch.Tensor, layer: int, need_dx: bool = True):
        """dy (N,B,E) of the attention output -> dx of its input; accumulates the adapter gradients of ``layer`` into ``grads``."""
        dy, dx, B = self._dy_dx(dy_nbe, need_dx)
        _lib.check(self.lib.pevit_attention_backward(self._ctx, _lib.stream_ptr(), layer, _lib.ptr(dy), _lib.ptr(dx), B), "pevit_attention_backward")
        return dx

    def transformer_backward(self, dy_nbe: torch.Tensor, need_dx: bool = True):
        dy, dx, B = self._dy_dx(dy_nbe, need_dx)
        _lib.check(self.lib.pevit_transformer_backward(self._ctx, _lib.stream_ptr(), _lib.ptr(dy), _lib.ptr(dx), B), "pevit_transformer_backward")
        return dx

    # ------------------------------------------------------------------ images in: the whole tower in one engine call
    def _walk_input(self, images, entry):
        """What every whole-tower walk from pixels does before its engine call: flush a pipelined DP step (it may still owe the
        parameter update), resize and check the batch, bump the generations.  Returns (pixels as the engine reads them, B, the
        C entry ``entry`` in their form)."""
        self.dp_flush()
        img = self._pixels(images)
        self._check_batch(img)
        self._begin_forward(range(self.arch.layers), flush=False)
        return img, img.shape[0], self._entry(entry, img)

    def visual_forward(self, images: torch.Tensor, save: bool = True) -> torch.Tensor:
        img, B, fn = self._walk_input(images, "pevit_visual_forward")
        feat = self._empty(B, self.arch.embed_dim)
        _lib.check(fn(self._ctx, _lib.stream_ptr(), _lib.ptr(img), _lib.ptr(feat), B, int(save)), "pevit_visual_forward")
        return feat

    def predict(self, images: torch.Tensor, logits_out=None, return_features: bool = False):
        """images -> logits in ONE engine call, for evaluation (``pevit_predict``): the tower in its inference form (nothing is
        stored for a backward pass), BatchNorm1d in eval mode on ``running_mean`` / ``running_var``, the Linear head.  Bit-identical
        to ``head_forward_backward(visual_forward(images, save=False), None, bn_training=False)[0]``; parameters, gradients,
        momentum and the running statistics are only read.  Returns the logits (B, C) as a device tensor without synchronising --
        ``logits_out``: a caller-owned f32 destination -- and ``(logits, features (B, D))`` with ``return_features``.  Like every
        forward it invalidates the activations a pending backward would read."""
        img, B, fn = self._walk_input(images, "pevit_predict")
        logits = self._out_or_new(logits_out, (B, self.num_classes))
        feat = self._empty(B, self.arch.embed_dim) if return_features else None
        _lib.check(fn(self._ctx, _lib.stream_ptr(), _lib.ptr(img), _lib.ptr(self.running_mean), _lib.ptr(self.running_var),
                      _lib.ptr(logits), _lib.ptr(feat), B), "pevit_predict")
        return (logits, feat) if return_features else logits

    def encode_image(self, images: torch.Tensor) -> torch.Tensor:
        """images -> features (B, D) through the inference forms of the tower, without a head (``pevit_encode_image``;
        CLIP.encode_image for evaluation).  The bits ``predict(..., return_features=True)`` returns; nothing is stored for a
        backward pass; no synchronise."""
        img, B, fn = self._walk_input(images, "pevit_encode_image")
        feat = self._empty(B, self.arch.embed_dim)
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
        if not self._fits(text_cd, torch.float32, (None, D)):
            self._refuse(text_cd, f"text_cd must be a contiguous float32 tensor (C, {D})")
        img, B, fn = self._walk_input(images, "pevit_zeroshot")
        Cc = text_cd.shape[0]
        probs = self._out_or_new(probs_out, (B, Cc))
        logits = self._empty(B, Cc) if return_logits else None
        feat = self._empty(B, D) if return_features else None
        _lib.check(fn(self._ctx, _lib.stream_ptr(), _lib.ptr(img), _lib.ptr(text_cd), Cc, float(scale), _lib.ptr(probs),
                      _lib.ptr(logits), _lib.ptr(feat), B), "pevit_zeroshot")
        out = (probs,) + ((logits,) if return_logits else ()) + ((feat,) if return_features else ())
        return out if len(out) > 1 else probs

    # ------------------------------------------------------------------ linear probe on cached features (csrc/probe.hip)
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
        a = self._probe_args
        if a is None or self._probe_seen != seen:
            bce = self._check_cache(feats, None, labels)
            a = self._probe_args = _lib.PevitProbeArgs()
            a.feat, a.rows = feats.data_ptr(), feats.shape[0]
            a.labels, a.targets = (None, labels.data_ptr()) if bce else (labels.data_ptr(), None)
            a.running_mean, a.running_var = self.running_mean.data_ptr(), self.running_var.data_ptr()
            self._probe_seen = seen
        self._check_index(index)
        B = index.shape[0]
        if update and self._optim_kind not in (None, "sgd"):
            raise _lib.PevitError(f"probe_step: the optimizer state belongs to {self._optim_kind!r}; call reset_optimizer() first")
        if not 2 <= B <= self.max_batch:
            raise _lib.PevitError(f"probe_step: batch {B} outside [2, {self.max_batch}] (max_batch of the bound workspace)")
        logits, loss = self._step_out(B, logits_out, loss_out)
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
        logits = self._out_or_new(logits_out, (n, self.num_classes))
        a = _lib.PevitProbePredictArgs()
        a.feat, a.rows = feats.data_ptr(), feats.shape[0]
        a.index_or_null = None if index is None else index.data_ptr()
        a.first_row, a.count = int(first_row), int(n)
        a.running_mean, a.running_var = self.running_mean.data_ptr(), self.running_var.data_ptr()
        a.scale, a.logits = float(scale), logits.data_ptr()
        _lib.check(self.lib.pevit_probe_predict(self._ctx, _lib.stream_ptr(), C.byref(a)), "pevit_probe_predict")
        return logits

    # ------------------------------------------------------------------ the training step and its seams
    def visual_backward(self, dfeat: torch.Tensor):
        self.dp_flush()
        d = dfeat.contiguous().float()
        _lib.check(self.lib.pevit_visual_backward(self._ctx, _lib.stream_ptr(), _lib.ptr(d), d.shape[0]), "pevit_visual_backward")

    def head_forward_backward(self, feat, labels, bn_training=True, need_dfeat=True, out=None):
        """BatchNorm1d -> Linear -> loss, forward and backward.  ``labels``: int64 (B,) -> cross-entropy, float32 (B, num_classes)
        -> BCEWithLogitsLoss, None -> forward only.  ``out``: caller-owned f32 (logits (B, C), loss (1,), dfeat like ``feat``)
        instead of fresh tensors.  A batch larger than that of the last saving forward lays the workspace out afresh: a backward
        through that forward is refused afterwards."""
        self.dp_flush()
        B = feat.shape[0]
        fn = self.lib.pevit_head_forward_backward if labels is None else self._head_fn(labels, B)
        logits, loss, dfeat = out or (self._empty(B, self.num_classes), torch.zeros(1, dtype=torch.float32, device=self.device),
                                      torch.empty_like(feat) if (need_dfeat and labels is not None) else None)
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
        self._begin_forward((), flush=False)          # the pipelined schedule: the call itself waits, behind its stem
        logits, loss = self._step_out(B, logits_out, loss_out)
        fn = self._train_fn(images, bce)
        _lib.check(fn(self._ctx, _lib.stream_ptr(), _lib.ptr(images), _lib.ptr(labels), _lib.ptr(self.running_mean),
                      _lib.ptr(self.running_var), int(bn_training), _lib.ptr(logits), _lib.ptr(loss), B),
                   "pevit_train_forward_backward")
        return logits, loss

    def train_step(self, images, labels, lr=None, momentum=0.9, weight_decay=0.0, bn_training=True, process_group=None,
                   world_size=1, nesterov=False, logits_out=None, loss_out=None, optimizer=None):
        """One reference ``train_one`` iteration (kadaptation_clip.py:347-353).  With DP the flat gradient buffer
        is the only thing that crosses xGMI (the frozen backbone never does); how it is exchanged is ``dp_exchange_mode``
        (default: one in-stream all-reduce behind the fused forward/backward call, 1/world folded into the SGD kernel).
        ``optimizer``: an ``OptimPlan`` (Adam, AdamW, SGD with several groups) -- the update is then ``optimizer_step(plan)``
        wherever it is ``sgd_step`` otherwise, and ``lr`` / ``momentum`` / ``weight_decay`` / ``nesterov`` are not read.
        With ``self.max_grad_norm`` set the gradients are clipped to that L2 norm right in front of the update (two more launches,
        no host read; under DP behind the exchange, on the norm of the averaged gradient); None, the default: the launches of before."""
        if optimizer is None and lr is None:
            raise TypeError("train_step: lr (plain SGD) or optimizer (an OptimPlan) is required")
        if world_size > 1:
            return self._train_step_dp(images, labels, lr, momentum, weight_decay, bn_training, process_group, world_size,
                                       nesterov, logits_out, loss_out, optimizer)
        logits, loss = self.forward_backward(images, labels, bn_training, logits_out, loss_out)
        self._update(optimizer, lr, momentum, weight_decay, 1.0, nesterov)
        return logits, loss

    # ------------------------------------------------------------------ per-launch profile (csrc/profile.hip)
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
