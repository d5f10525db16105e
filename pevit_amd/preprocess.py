"""Host restatement of the reference's ``Resize(n_px, bicubic) + CenterCrop`` on uint8 pixels (clip_load._Preprocess), in integers.

Pillow's 8-bit resize is an exact algorithm: per axis a table of fixed-point taps (``precompute_coeffs`` + ``normalize_coeffs_8bpc``
of its Resample.c, double arithmetic in one fixed order, 22 fractional bits), a horizontal pass that rounds to uint8, and a
vertical pass over those bytes.  Restated here with numpy so that

* the engine's resize kernel (csrc/resize.hip) and its planner (csrc/resize_plan.hip) have an oracle that needs no Pillow, and
* the loader can resize a native-size archive on the host (``DATASET.RESIZE_ON_HOST``, ``DATASET.NORMALIZE_ON_HOST``).

``tests/test_resize_host.py`` holds it to ``Image.resize(..., Image.BICUBIC)`` byte for byte.

The second half of the file is the geometry PER IMAGE: ``resize_u8(images, n, center_crop)`` adds the reference's
``DATASET.CENTER_CROP False`` (``Resize((n, n))``, nothing cropped), and ``RaggedImages`` / ``RaggedBatch`` describe a set whose
pictures all differ in size the way the engine's ragged resize reads it (csrc/resize_ragged.hip): one pool of pixels, one
descriptor per image, one table pair per distinct axis.  ``tests/test_resize_ragged_host.py``.
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


# ---- one geometry per image: the squash mode of DATASET.CENTER_CROP False, and ragged sets (csrc/resize_ragged.hip) ---------------
KERNEL_MAX_SIDE, KERNEL_MAX_TAPS, KERNEL_MAX_OUT = 4096, 33, 256       # what the resize kernels take (csrc/resize.hip)


def axis_keys(h: int, w: int, n: int, center_crop: bool = True):
    """The two axis keys ``(in_size, out_size, first)`` of an (h, w) source and target ``n``, horizontal then vertical; ``n`` rows of
    each are used.  ``center_crop``: the geometry of ``resize_geometry``; otherwise the reference's ``Resize((n, n))`` of
    ``DATASET.CENTER_CROP False`` (feature.py:543-549): both axes go to ``n`` and nothing is cropped."""
    if center_crop:
        nh, nw, top, left = resize_geometry(h, w, n)
        return (int(w), nw, left), (int(h), nh, top)
    if int(h) < 1 or int(w) < 1 or int(n) < 1:
        raise ValueError(f"axis_keys: sizes must be positive, got h={h} w={w} n={n}")
    return (int(w), int(n), 0), (int(h), int(n), 0)


def in_kernel_range(h: int, w: int, n: int, center_crop: bool = True) -> bool:
    """True when the resize kernels take an (h, w) source: sides up to 4096 and at most 33 taps per sample on either axis."""
    (_, nw, _), (_, nh, _) = axis_keys(h, w, n, center_crop)
    return max(h, w) <= KERNEL_MAX_SIDE and max(axis_ksize(w, nw), axis_ksize(h, nh)) <= KERNEL_MAX_TAPS


def resize_u8(images, n: int, center_crop: bool = True):
    """uint8 (B, 3, h, w) -> uint8 (B, 3, n, n).  ``center_crop`` True: ``resize_center_crop_u8``.  False: Pillow's
    ``resize((n, n), BICUBIC)`` of every plane, the whole picture squashed and nothing cropped.  torch in, torch out."""
    if center_crop:
        return resize_center_crop_u8(images, n)
    is_torch = not isinstance(images, np.ndarray)
    x = images.detach().cpu().numpy() if is_torch else images
    if x.dtype != np.uint8 or x.ndim != 4:
        raise ValueError(f"resize_u8: expected uint8 (B, C, h, w), got {x.dtype} {x.shape}")
    h, w = x.shape[2:]
    kh, bh = resample_axis(w, n)
    kv, bv = resample_axis(h, n)
    out = np.ascontiguousarray(resample_pass(resample_pass(x, kh, bh, axis=3), kv, bv, axis=2))
    if is_torch:
        import torch
        return torch.from_numpy(out)
    return out


# numpy twin of pevit_resize_ragged_desc (include/pevit_hip.h): 40 bytes, no padding
RAGGED_DESC = np.dtype([("offset", "<i8"), ("h", "<i4"), ("w", "<i4"), ("kh_off", "<i4"), ("bh_off", "<i4"), ("ksize_h", "<i4"),
                        ("kv_off", "<i4"), ("bv_off", "<i4"), ("ksize_v", "<i4")])
assert RAGGED_DESC.itemsize == 40


def ragged_offsets(shapes) -> np.ndarray:
    """Byte offsets of the dense (3, h, w) blocks of a pool, int64, one more entry than images: the running sum of 3 h w."""
    s = np.asarray(shapes).astype(np.int64).reshape(-1, 2)
    off = np.zeros(len(s) + 1, dtype=np.int64)
    np.cumsum(3 * s[:, 0] * s[:, 1], out=off[1:])
    return off


def ragged_image(pool, shapes, offsets, i):
    """Image ``i`` of a pool as a (3, h, w) view."""
    h, w = int(shapes[i][0]), int(shapes[i][1])
    return pool[int(offsets[i]):int(offsets[i]) + 3 * h * w].reshape(3, h, w)


def resize_ragged_u8(pool, shapes, n: int, center_crop: bool = True) -> np.ndarray:
    """A ragged pool -> dense uint8 (N, 3, n, n), image by image through ``resize_u8``: the host route of a ragged set."""
    pool = np.asarray(pool)
    off = ragged_offsets(shapes)
    out = np.empty((len(shapes), 3, n, n), dtype=np.uint8)
    for i in range(len(shapes)):
        out[i] = resize_u8(ragged_image(pool, shapes, off, i)[None], n, center_crop)[0]
    return out


def _lib_axis_tables(lib, in_size, out_size, first, n):
    """Rows first .. first + n of one axis from the library's planner (pevit_resize_axis)."""
    import ctypes as C
    ks = lib.pevit_resize_axis(in_size, out_size, 0, 0, None, None)
    if ks < 1:
        raise ValueError(f"pevit_resize_axis: axis {in_size} -> {out_size} refused")
    k, b = np.empty((n, ks), dtype=np.int32), np.empty((n, 2), dtype=np.int32)
    if lib.pevit_resize_axis(in_size, out_size, first, n, C.c_void_p(k.ctypes.data), C.c_void_p(b.ctypes.data)) != 0:
        raise ValueError(f"pevit_resize_axis: rows [{first}, {first + n}) of axis {in_size} -> {out_size} refused")
    return k, b


def ragged_table_bytes(shapes, n: int, center_crop: bool = True) -> int:
    """Bytes of the deduplicated table pools of a set, without planning a table."""
    keys = set()
    for h, w in np.asarray(shapes).reshape(-1, 2).tolist():
        if in_kernel_range(h, w, n, center_crop):
            keys.update(axis_keys(h, w, n, center_crop))
        else:
            keys.add((n, n, 0))
    return sum(4 * n * (axis_ksize(i, o) + 2) for i, o, _ in keys)


class RaggedImages:
    """A uint8 image set with one size per image, as the engine's ragged resize reads it (csrc/resize_ragged.hip):

    * ``pool``     1-D uint8 tensor: the dense (3, h_i, w_i) blocks, one after the other;
    * ``desc``     (N, 10) int32 tensor, the bytes of N ``pevit_resize_ragged_desc`` (``host_desc``: the same as a RAGGED_DESC array);
    * ``k_pool`` / ``b_pool``  1-D int32 tensors: one (n, ksize) tap table and one (n, 2) bounds table per DISTINCT axis key
      ``(in_size, out_size, first)`` of the set, from the library's planner (``preprocess.resample_axis`` is its oracle).

    Images the kernel does not take (a side above 4096, an axis of more than 33 taps) are resized on the host when the set is
    built and stored as n x n blocks, whose axes are the one-tap identity.  ``len``, ``.to(device)`` and indexing by an index
    tensor or array, which gives a ``RaggedBatch`` and copies no pixel.  ``shape`` / ``dtype`` / ``device`` / ``numel`` answer as
    a (N, 3, 0, 0) uint8 tensor would where the loader asks (``sample_spec``, the resident-set budget)."""

    def __init__(self, pool, host_desc, k_pool, b_pool, out, center_crop, keys=None, pre_resized=0):
        import torch
        self.pool, self.k_pool, self.b_pool = pool, k_pool, b_pool
        self.host_desc = host_desc
        self.desc = torch.from_numpy(host_desc.view(np.int32).reshape(len(host_desc), 10).copy()).to(pool.device)
        self.out, self.center_crop = int(out), bool(center_crop)
        self.max_ksize_v = int(host_desc["ksize_v"].max())
        self.keys = keys or {}                       # axis key -> (k_off, b_off, ksize)
        self.pre_resized = int(pre_resized)

    @classmethod
    def build(cls, pool, shapes, n: int, center_crop: bool = True, lib=None):
        """From the archive's pool (1-D uint8, numpy or torch) and (N, 2) shapes.  The library's planner makes the tables and its
        ``pevit_resize_ragged_check`` validates the descriptors (both host code: no GPU is needed); ``lib``: the loaded library."""
        import ctypes as C
        import torch
        if lib is None:
            from . import _lib
            lib = _lib.load()
        pool = pool.numpy() if isinstance(pool, torch.Tensor) else np.asarray(pool)
        shapes = np.asarray(shapes).astype(np.int64).reshape(-1, 2)
        if pool.dtype != np.uint8 or pool.ndim != 1 or len(shapes) < 1:
            raise ValueError(f"RaggedImages: a 1-D uint8 pool and (N, 2) shapes, got {pool.dtype} {pool.shape} and {shapes.shape}")
        if not 1 <= int(n) <= KERNEL_MAX_OUT:
            raise ValueError(f"RaggedImages: target {n} outside [1, {KERNEL_MAX_OUT}]")
        if shapes.min() < 1:
            raise ValueError("RaggedImages: every side must be at least 1")
        off = ragged_offsets(shapes)
        if off[-1] != pool.size:
            raise ValueError(f"RaggedImages: the shapes describe {int(off[-1])} bytes, the pool holds {pool.size}")
        far = [i for i, (h, w) in enumerate(shapes.tolist()) if not in_kernel_range(h, w, n, center_crop)]
        if far:                                      # stored pre-resized: their blocks become n x n
            parts, last = [], 0
            shapes = shapes.copy()
            for i in far:
                parts += [pool[off[last]:off[i]], resize_u8(ragged_image(pool, shapes, off, i)[None], n, center_crop).reshape(-1)]
                last = i + 1
            parts.append(pool[off[last]:])
            pool = np.concatenate(parts)
            shapes[far] = n
            off = ragged_offsets(shapes)
        keys, ks, bs, k_len, b_len = {}, [], [], 0, 0
        desc = np.zeros(len(shapes), dtype=RAGGED_DESC)
        desc["offset"] = off[:-1]
        desc["h"], desc["w"] = shapes[:, 0], shapes[:, 1]
        for i, (h, w) in enumerate(shapes.tolist()):
            for axis, key in zip("hv", axis_keys(h, w, n, center_crop)):
                if key not in keys:
                    k, b = _lib_axis_tables(lib, *key, n)
                    keys[key] = (k_len, b_len, k.shape[1])
                    ks.append(k.reshape(-1)); bs.append(b.reshape(-1))
                    k_len += k.size; b_len += b.size
                desc[f"k{axis}_off"][i], desc[f"b{axis}_off"][i], desc[f"ksize_{axis}"][i] = keys[key]
        k_pool, b_pool = np.concatenate(ks).astype(np.int32), np.concatenate(bs).astype(np.int32)
        if lib.pevit_resize_ragged_check(C.c_void_p(desc.ctypes.data), len(desc), pool.size, k_pool.size, b_pool.size, int(n)) != 0:
            raise ValueError(lib.pevit_last_error().decode())
        return cls(torch.from_numpy(np.ascontiguousarray(pool)), desc, torch.from_numpy(k_pool), torch.from_numpy(b_pool), n,
                   center_crop, keys, len(far))

    # ---- what the loader asks of an image tensor
    def __len__(self):
        return len(self.host_desc)

    @property
    def device(self):
        return self.pool.device

    @property
    def dtype(self):
        return self.pool.dtype

    @property
    def shape(self):
        return (len(self), 3, 0, 0)                  # no common size: (0, 0) is never the tower's

    def numel(self):
        return self.pool.numel()

    def element_size(self):
        return 1

    @property
    def table_bytes(self):
        return 4 * (self.k_pool.numel() + self.b_pool.numel())

    def to(self, device, non_blocking=False):
        import torch
        device = torch.device(device)
        if device == self.pool.device:
            return self
        new = object.__new__(RaggedImages)
        new.__dict__.update(self.__dict__)
        for name in ("pool", "desc", "k_pool", "b_pool"):
            setattr(new, name, getattr(self, name).to(device))
        return new

    def __getitem__(self, index):
        import torch
        if isinstance(index, (int, np.integer)):
            index = [int(index)]
        index = torch.as_tensor(np.asarray(index) if not isinstance(index, torch.Tensor) else index, dtype=torch.int64)
        return RaggedBatch(self, index.to(self.pool.device).reshape(-1).contiguous())

    def subset(self, index):
        """The images ``index`` as a set of their own (the few-shot subset): the same pool and tables, their descriptors only."""
        import torch
        new = object.__new__(RaggedImages)
        new.__dict__.update(self.__dict__)
        new.host_desc = self.host_desc[np.asarray(index, dtype=np.int64)].copy()
        new.desc = torch.from_numpy(new.host_desc.view(np.int32).reshape(len(new.host_desc), 10).copy()).to(self.pool.device)
        new.max_ksize_v = int(new.host_desc["ksize_v"].max())
        return new

    def image(self, i):
        """Image ``i`` as stored: a (3, h, w) uint8 view of the pool."""
        d = self.host_desc[int(i)]
        return self.pool[int(d["offset"]):int(d["offset"]) + 3 * int(d["h"]) * int(d["w"])].view(3, int(d["h"]), int(d["w"]))

    def resize_on_host(self, index=None):
        """Dense uint8 (len(index), 3, out, out) on the host through ``resize_u8``, image by image: what the kernel gives."""
        import torch
        idx = range(len(self)) if index is None else [int(i) for i in torch.as_tensor(index).cpu().reshape(-1).tolist()]
        cpu = self.to("cpu")
        out = torch.empty((len(idx), 3, self.out, self.out), dtype=torch.uint8)
        for j, i in enumerate(idx):
            out[j] = resize_u8(cpu.image(i)[None].contiguous(), self.out, self.center_crop)[0]
        return out


class RaggedBatch:
    """A batch of a ``RaggedImages`` set: the set (pool, descriptors, tables -- shared, not copied) and the int64 ``index`` of its
    images on the set's device.  Travels wherever a uint8 image batch travels: it answers ``shape`` (B, 3, 0, 0), ``dtype``,
    ``device``, ``dim()``, ``size()``, ``contiguous()`` and ``to()`` like one, and ``HipEngine._input`` turns it into the dense
    (B, 3, R, R) batch with one ``pevit_resize_ragged_u8`` launch."""

    def __init__(self, images: RaggedImages, index):
        self.images, self.index = images, index

    pool = property(lambda self: self.images.pool)
    desc = property(lambda self: self.images.desc)
    k_pool = property(lambda self: self.images.k_pool)
    b_pool = property(lambda self: self.images.b_pool)
    out = property(lambda self: self.images.out)
    center_crop = property(lambda self: self.images.center_crop)
    max_ksize_v = property(lambda self: self.images.max_ksize_v)
    device = property(lambda self: self.images.device)
    dtype = property(lambda self: self.images.dtype)
    shape = property(lambda self: (int(self.index.shape[0]), 3, 0, 0))

    def __len__(self):
        return int(self.index.shape[0])

    def dim(self):
        return 4

    def size(self, i=None):
        return self.shape if i is None else self.shape[i]

    def is_contiguous(self):
        return True

    def contiguous(self):
        return self

    def to(self, device, non_blocking=False):
        images = self.images.to(device)
        return self if images is self.images else RaggedBatch(images, self.index.to(images.device))

    def resize_on_host(self):
        return self.images.resize_on_host(self.index)
