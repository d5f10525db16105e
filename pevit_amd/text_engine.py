"""Host-side owner of one text-tower context of the HIP engine (include/pevit_hip.h: pevit_text_create / pevit_encode_text).

``CLIP.encode_text`` (model.py:1153-1168) -- token embedding + positional embedding, the causal transformer, ``ln_final`` on the
end-of-text row, ``@ text_projection`` -- as ONE engine call per chunk of prompts.  The context is inference-only: its workspace
holds the inference layout, and nothing differentiates through it.  There is no PyTorch fallback: without the library or a GPU
the constructor raises.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._context import EngineContext
from .synth import VitArch

TEXT_WEIGHT_FORMATS = ("bf16", "f32-verify")
MAX_CONTEXT = 128        # attn_causal.hip keeps K and V of a prompt in LDS
_INT_DTYPES = (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8)


def text_engine_refusal(model) -> str | None:
    """Why ``model``'s text tower cannot run on the engine (None: it can).  Pure: reads shapes, devices and flags only."""
    width = int(model.token_embedding.weight.shape[1])
    embed_dim = int(model.text_projection.shape[1])
    if width % 128 != 0 or width > 1024:
        return f"text width {width} is not a multiple of 128 in (0, 1024]"
    if int(model.context_length) > MAX_CONTEXT or int(model.context_length) < 1:
        return f"context_length {int(model.context_length)} outside [1, {MAX_CONTEXT}]"
    if embed_dim % 8 != 0:
        return f"embed_dim {embed_dim} is not a multiple of 8"
    if not model.token_embedding.weight.is_cuda:
        return "the model is not on a GPU"
    for name, p in text_tower_parameters(model):
        if p.requires_grad:
            return f"text-tower parameter {name} requires a gradient (the engine's text tower is frozen, forward only)"
    return None


def text_engine_ok(model) -> bool:
    """True when the engine can stand in for ``model.encode_text``: width a multiple of 128 up to 1024, context_length <= 128,
    embed_dim a multiple of 8, the model on a GPU and no trainable parameter in the text tower."""
    return text_engine_refusal(model) is None


def text_tower_parameters(model):
    """(name, parameter) of everything ``encode_text`` reads."""
    for n, p in model.transformer.named_parameters():
        yield "transformer." + n, p
    yield "token_embedding.weight", model.token_embedding.weight
    yield "positional_embedding", model.positional_embedding
    for n, p in model.ln_final.named_parameters():
        yield "ln_final." + n, p
    yield "text_projection", model.text_projection


class TextEngine(EngineContext):
    def __init__(self, arch: VitArch, max_prompts: int = 256, device: str | torch.device = "cuda:0", weight_format: str = "bf16"):
        super().__init__(device)
        if weight_format not in TEXT_WEIGHT_FORMATS:
            raise _lib.PevitError(f"TextEngine: weight_format {weight_format!r}: the text tower takes one of {TEXT_WEIGHT_FORMATS}")
        if max_prompts < 1:
            raise _lib.PevitError(f"TextEngine: max_prompts {max_prompts} must be positive")
        self.arch, self.max_prompts, self.weight_format = arch, int(max_prompts), weight_format
        dims = _lib.PevitTextDims(arch.text_width, arch.text_layers, arch.context_length, arch.vocab_size, arch.embed_dim,
                                  _lib.WEIGHT_FORMATS[weight_format])
        self._create("pevit_text_create", dims, self.max_prompts)

    def load_state_dict(self, sd):
        """Frozen text tower from an OpenAI-layout state-dict (any float dtype, any device): ``transformer.resblocks.*``,
        ``token_embedding.weight``, ``positional_embedding``, ``ln_final.*`` and ``text_projection``."""
        a = self.arch
        want = {"token_embedding.weight": (a.vocab_size, a.text_width), "positional_embedding": (a.context_length, a.text_width),
                "text_projection": (a.text_width, a.embed_dim)}
        for k, shape in want.items():
            if tuple(sd[k].shape) != shape:
                raise _lib.PevitError(f"TextEngine.load_state_dict: {k} has shape {tuple(sd[k].shape)}, expected {shape}")
        keep = self._load_blocks(sd, "", a.text_layers)
        ts = [self._dev(sd[k]) for k in ("token_embedding.weight", "positional_embedding", "ln_final.weight", "ln_final.bias",
                                         "text_projection")]
        keep.append(ts)
        _lib.check(self.lib.pevit_load_text_stem(self._ctx, _lib.stream_ptr(), *[_lib.ptr(t) for t in ts]), "pevit_load_text_stem")
        torch.cuda.current_stream().synchronize()     # the temporaries above may now be freed
        del keep

    def encode(self, tokens: torch.Tensor) -> torch.Tensor:
        """tokens (S, context_length), any integer dtype, on the CPU or the device -> text features (S, D) f32 on the device.
        Sets larger than ``max_prompts`` are split into calls of at most that many prompts.  The launches are left on the current
        stream: the caller synchronises when it reads the result."""
        a = self.arch
        if not torch.is_tensor(tokens) or tokens.dim() != 2 or tokens.shape[1] != a.context_length:
            shape = tuple(tokens.shape) if torch.is_tensor(tokens) else type(tokens).__name__
            raise _lib.PevitError(f"TextEngine.encode: tokens of shape {shape}, expected (S, {a.context_length})")
        if tokens.dtype not in _INT_DTYPES:
            raise _lib.PevitError(f"TextEngine.encode: tokens of dtype {tokens.dtype}, expected an integer dtype")
        S = tokens.shape[0]
        out = torch.empty((S, a.embed_dim), dtype=torch.float32, device=self.device)
        if S == 0:
            return out
        # the range is checked here, on the host (the embedding kernel clamps, it never reads outside the table): before the
        # upload for host tensors, with one aminmax for device tensors
        lo, hi = (int(v) for v in torch.aminmax(tokens))
        if lo < 0 or hi >= a.vocab_size:
            raise _lib.PevitError(f"TextEngine.encode: token ids in [{lo}, {hi}] outside the vocabulary [0, {a.vocab_size - 1}]")
        tok = tokens.to(device=self.device, dtype=torch.int64).contiguous()
        s = _lib.stream_ptr()
        N, D = a.context_length, a.embed_dim
        for i in range(0, S, self.max_prompts):
            n = min(self.max_prompts, S - i)
            _lib.check(self.lib.pevit_encode_text(self._ctx, s, C.c_void_p(tok.data_ptr() + i * N * 8),
                                                  C.c_void_p(out.data_ptr() + i * D * 4), n), "pevit_encode_text")
        return out
