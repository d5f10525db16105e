"""Host restatement of the reference's ``Resize(n_px, bicubic) + CenterCrop`` on uint8 pixels (clip_load._Preprocess), in integers.

Pillow's 8-bit resize is an exact algorithm: per axis a table of fixed-point taps (``precompute_coeffs`` + ``normalize_coeffs_8bpc``
of its Resample.c, double arithmetic in one fixed order, 22 fractional bits), a horizontal pass that rounds to uint8, and a
vertical pass over those bytes.  Restated here with numpy so that

* the engine's resize kernel (csrc/resize.hip) and its planner (csrc/resize_plan.hip) have an oracle that needs no Pillow, and
* the loader can resize a native-size archive on the host (``DATASET.RESIZE_ON_HOST``, ``DATASET.NORMALIZE_ON_HOST``).

``tests/test_resize_host.py`` holds it to ``Image.resize(..., Image.BICUBIC)`` byte for byte.
"""
from __future__ import annotations

import math

import numpy as np

PRECISION_BITS = 22          # Pillow: 32 - 8 - 2
_A = -0.5                    # the bicubic kernel's parameter in Pillow (-0.75 is OpenCV's)


def resize_geometry(h: int, w: int, n: int):
    """(nh, nw, top, left) of clip_load._Preprocess for an (h, w) source and target ``n``: the shorter side becomes ``n``, the
    other ``int(n * longer / shorter)``; the crop window starts at the half-to-even rounded half difference."""
    h, w, n = int(h), int(w), int(n)
    if h < 1 or w < 1 or n < 1:
        raise ValueError(f"resize_geometry: sizes must be positive, got h={h} w={w} n={n}")
    if w <= h:
        nw, nh = n, int(n * h / w)
    else:
        nw, nh = int(n * w / h), n
    return nh, nw, int(round((nh - n) / 2.0)), int(round((nw - n) / 2.0))


def _bicubic(t: float, a: float = _A) -> float:
    t = -t if t < 0.0 else t
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


def axis_ksize(in_size: int, out_size: int) -> int:
    """Taps per table row: 1 for an axis that is not resampled, Pillow's ``ksize`` otherwise."""
    if in_size == out_size:
        return 1
    fs = max(in_size / out_size, 1.0)
    return int(math.ceil(2.0 * fs)) * 2 + 1


def resample_axis(in_size: int, out_size: int, first: int = 0, count: int | None = None, a: float = _A, normalise: bool = True):
    """Rows ``first .. first + count`` of one axis' tables: ``k`` int32 (count, ksize) fixed-point taps, zero past each row's tap
    count, and ``bounds`` int32 (count, 2) = (first source sample, taps).  An axis of equal size is not resampled (Pillow skips
    that pass; a bicubic pass at equal size is not the identity): its table is the single tap 2^22 at the sample itself.
    (``a`` and ``normalise`` exist for the tests' wrong variants only.)"""
    in_size, out_size, first = int(in_size), int(out_size), int(first)
    count = out_size - first if count is None else int(count)
    if in_size < 1 or out_size < 1 or first < 0 or count < 1 or first + count > out_size:
        raise ValueError(f"resample_axis: rows [{first}, {first + count}) of an axis {in_size} -> {out_size}")
    ksize = axis_ksize(in_size, out_size)
    k = np.zeros((count, ksize), dtype=np.int32)
    bounds = np.zeros((count, 2), dtype=np.int32)
    if in_size == out_size:
        k[:, 0] = 1 << PRECISION_BITS
        bounds[:, 0] = np.arange(first, first + count)
        bounds[:, 1] = 1
        return k, bounds
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ss = 1.0 / fs
    for i in range(count):
        center = (first + i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss, a) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            v = w[x] / ww if (normalise and ww != 0.0) else w[x]
            k[i, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[i] = (xmin, xmax)
    return k, bounds


def resample_pass(x: np.ndarray, k: np.ndarray, bounds: np.ndarray, axis: int) -> np.ndarray:
    """One 8-bit pass along ``axis`` of a uint8 array: out = clamp((2^21 + sum p * k) >> 22, 0, 255), the shift arithmetic."""
    x = np.moveaxis(np.asarray(x), axis, -1)
    in_size, (count, ksize) = x.shape[-1], k.shape
    taps = np.arange(ksize, dtype=np.int64)[None, :]
    idx = np.minimum(bounds[:, :1].astype(np.int64) + taps, in_size - 1)              # (count, ksize); taps past the count are 0
    kk = np.where(taps < bounds[:, 1:2], k, 0).astype(np.int32)
    out = np.empty(x.shape[:-1] + (count,), dtype=np.uint8)
    flat_in, flat_out = x.reshape(-1, in_size), out.reshape(-1, count)
    step = max(1, (1 << 24) // max(1, count * ksize))                                  # rows per chunk: ~64 MB of int32 at most
    for lo in range(0, flat_in.shape[0], step):
        p = flat_in[lo:lo + step][:, idx].astype(np.int32)                            # (rows, count, ksize)
        s = (p * kk[None]).sum(axis=-1, dtype=np.int32) + np.int32(1 << (PRECISION_BITS - 1))
        flat_out[lo:lo + step] = np.clip(s >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, -1, axis)


def resize_center_crop_u8(images, n: int):
    """uint8 (B, 3, h, w) -> uint8 (B, 3, n, n): Pillow's bicubic resize of every plane to the geometry of ``resize_geometry``,
    cropped to the centre window.  Only the window's rows and columns are computed.  torch in, torch out; numpy in, numpy out."""
    is_torch = not isinstance(images, np.ndarray)
    x = images.detach().cpu().numpy() if is_torch else images
    if x.dtype != np.uint8 or x.ndim != 4:
        raise ValueError(f"resize_center_crop_u8: expected uint8 (B, C, h, w), got {x.dtype} {x.shape}")
    h, w = x.shape[2:]
    nh, nw, top, left = resize_geometry(h, w, n)
    kh, bh = resample_axis(w, nw, left, n)
    kv, bv = resample_axis(h, nh, top, n)
    lo, hi = int(bv[:, 0].min()), int((bv[:, 0] + bv[:, 1]).max())                     # the source rows the window reads
    mid = resample_pass(x[:, :, lo:hi, :], kh, bh, axis=3)                             # horizontal first, rounded to uint8
    bv = bv.copy(); bv[:, 0] -= lo
    out = np.ascontiguousarray(resample_pass(mid, kv, bv, axis=2))
    if is_torch:
        import torch
        return torch.from_numpy(out)
    return out
