"""What every host-side owner of an engine context does (include/pevit_hip.h): create the context, allocate the weight arena and
the activation workspace as torch tensors and bind them, bind again when the workspace grows, destroy the context with the owner,
load the frozen transformer blocks of an OpenAI-layout state-dict -- and say whether a tensor is what a raw pointer may read."""
import ctypes as C

import torch

from . import _lib

BLOCK_KEYS = ("attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias", "ln_1.weight", "ln_1.bias",
              "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias", "ln_2.weight", "ln_2.bias")


class EngineContext:
    def __init__(self, device):
        if not torch.cuda.is_available():
            raise _lib.PevitError(f"{type(self).__name__} needs a ROCm GPU (gfx950); there is no CPU fallback")
        self.lib = _lib.load()
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self._ctx = C.c_void_p()
        self.arena = self.workspace = None

    def _create(self, creator: str, dims, batch: int):
        _lib.check(getattr(self.lib, creator)(C.byref(dims), C.byref(self._ctx)), creator)
        self.arena = torch.zeros(self.lib.pevit_arena_bytes(self._ctx), dtype=torch.uint8, device=self.device)
        self._bind(batch)

    def _bind(self, batch: int):
        """A workspace for ``batch`` images (prompts) replaces the current one; the weights in the arena stay."""
        self.workspace = None
        self.workspace = torch.empty(self.lib.pevit_workspace_bytes(self._ctx, batch), dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.pevit_bind(self._ctx, _lib.ptr(self.arena), self.arena.numel(), _lib.ptr(self.workspace),
                                       self.workspace.numel(), batch), "pevit_bind")

    def __del__(self):
        try:
            if getattr(self, "_ctx", None):
                self.lib.pevit_ctx_destroy(self._ctx)
                self._ctx = None
        except Exception:
            pass

    def _dev(self, t):
        return t.detach().to(device=self.device, dtype=torch.float32).contiguous()

    def _load_blocks(self, sd, prefix: str, layers: int) -> list:
        """``{prefix}transformer.resblocks.0 .. layers-1`` into the arena; returns the f32 temporaries, which must outlive the
        copies enqueued on the current stream."""
        keep, s = [], _lib.stream_ptr()
        for i in range(layers):
            ts = [self._dev(sd[f"{prefix}transformer.resblocks.{i}.{k}"]) for k in BLOCK_KEYS]
            keep.append(ts)
            _lib.check(self.lib.pevit_load_block(self._ctx, s, i, *[_lib.ptr(t) for t in ts]), "pevit_load_block")
        return keep

    def _fits(self, t, dtype, shape) -> bool:
        """The tensor contract of the C ABI's raw pointers: ``t`` on this device, of ``dtype``, contiguous, of ``shape`` (None: any
        extent)."""
        return t.device == self.device and t.dtype == dtype and t.is_contiguous() and t.dim() == len(shape) and \
            all(want is None or want == have for want, have in zip(shape, t.shape))

    def _refuse(self, t, what: str, also: str = ""):
        raise _lib.PevitError(f"{what} on {self.device}{also}; got {tuple(t.shape)} {t.dtype} on {t.device}")
