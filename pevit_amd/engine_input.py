"""The uint8 input path of ``HipEngine``: the normalisation constants of the patch gather, and native-size or ragged uint8
batches resized on the GPU to the tower's resolution (csrc/resize.hip, csrc/resize_ragged.hip) before they take the unchanged
uint8 entries.  A mixin: its state (``_input_norm``, ``_input_resize``, ``_resize_center_crop``, ``_resize_buf``,
``_resize_cache``) is declared in ``HipEngine.__init__``."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .preprocess import RaggedBatch


class InputMixin:
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
        self._input_resize, self._resize_center_crop = bool(on), bool(center_crop)

    def _resize_tables(self, h, w):
        """Device tables of the (h, w) -> (R, R) resize + crop, planned by the library and uploaded once per source size."""
        cache, crop = self._resize_cache, self._resize_center_crop
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

    def _resize_staging(self, B):
        """The first ``B`` images of the staging tensor (``max_batch`` images: on first use, and again after ``ensure_batch``)."""
        if self._resize_buf is None:
            self._resize_buf = torch.empty((self.max_batch, 3) + (self.arch.resolution,) * 2, dtype=torch.uint8, device=self.device)
        return self._resize_buf[:B]

    def _resize_ragged(self, batch) -> torch.Tensor:
        """A ``preprocess.RaggedBatch`` on this device -> uint8 (B,3,R,R) in ONE launch (``pevit_resize_ragged_u8``), bit for bit
        ``preprocess.resize_u8`` of every image; a view of the resize staging tensor, like ``resize_u8``'s result."""
        R, crop = self.arch.resolution, self._resize_center_crop
        if batch.device != self.device or batch.index.dtype != torch.int64 or not batch.index.is_contiguous() or len(batch) < 1:
            raise _lib.PevitError(f"resize_u8: a ragged batch must live on {self.device} with a contiguous int64 index of at least "
                                  f"one image; got {len(batch)} images on {batch.device}")
        if batch.out != R or batch.center_crop != crop:
            raise _lib.PevitError(f"resize_u8: the ragged set was planned for a {batch.out} x {batch.out} tower with center_crop="
                                  f"{batch.center_crop}; this engine resizes to {R} x {R} with center_crop={crop}")
        B = len(batch)
        self._check_bound(B)
        out = self._resize_staging(B)
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
        if not self._fits(images, torch.uint8, (None, 3, None, None)) or images.shape[0] < 1:
            self._refuse(images, "resize_u8: images must be a contiguous uint8 tensor (B,3,h,w)")
        B, _, h, w = images.shape
        self._check_bound(B)
        kh, bh, ksh, kv, bv, ksv = self._resize_tables(int(h), int(w))
        out = self._resize_staging(B)
        R = self.arch.resolution
        _lib.check(self.lib.pevit_resize_u8(_lib.stream_ptr(), _lib.ptr(images), 3 * B, h, w, _lib.ptr(out), R, R, _lib.ptr(kh),
                                            _lib.ptr(bh), ksh, _lib.ptr(kv), _lib.ptr(bv), ksv), "pevit_resize_u8")
        return out

    def _needs_resize(self, images) -> bool:
        return isinstance(images, RaggedBatch) or (self._input_resize and self._input_norm is not None and images.dtype == torch.uint8
            and images.dim() == 4 and tuple(images.shape[2:]) != (self.arch.resolution,) * 2)

    def _input(self, images):
        """The ONE place a native-size uint8 batch becomes (B,3,R,R): every uint8-taking method passes its images through here
        and then through its unchanged checks and its unchanged ``_u8`` entry.  Anything else comes back as it is.  A ragged batch
        (``preprocess.RaggedBatch``) can only be resized: it is refused where a native-size batch would be."""
        if isinstance(images, RaggedBatch) and not (self._input_resize and self._input_norm is not None):
            raise _lib.PevitError("a ragged uint8 batch needs set_input_normalization(mean, std) and set_input_resize(True)")
        return self.resize_u8(images) if self._needs_resize(images) else images

    def _pixels(self, images):
        """What the seams and the inference walks hand to the engine: uint8 pixels through ``_input``, anything else as f32."""
        return self._input(images.contiguous()) if images.dtype == torch.uint8 else images.contiguous().float()
