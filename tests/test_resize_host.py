"""The uint8 resize without a GPU: the numpy restatement (pevit_amd/preprocess.py) against Pillow byte for byte, the library's
planner (csrc/resize_plan.hip) against the restatement table for table, the refusals of ``pevit_resize_u8`` and the loader's routes.

The restatement is the oracle of tests/test_gpu_resize.py; ``GPU_SOURCES`` / ``GPU_TARGETS`` is that test's list, and the mutant
test below shows that on this list a wrong kernel of each kind cannot pass."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from pevit_amd import _lib, preprocess as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (source h, w) -> (resized h, w), plain resizes without a crop
SIZE_PAIRS = [((32, 32), (224, 224)), ((28, 28), (224, 224)), ((8, 8), (224, 224)), ((64, 64), (224, 224)), ((96, 96), (224, 224)),
              ((256, 256), (224, 224)), ((448, 448), (224, 224)),
              ((90, 60), (72, 48)), ((53, 37), (320, 224)), ((500, 300), (373, 224)), ((384, 512), (224, 298)),
              ((700, 1000), (224, 320)),
              ((48, 48), (32, 32)), ((47, 33), (23, 16)), ((5, 7), (2, 3))]
GPU_SOURCES = [(8, 8), (32, 32), (37, 53), (53, 37), (48, 55), (96, 96), (384, 384)]      # (h, w) of tests/test_gpu_resize.py
GPU_TARGETS = (48, 64)


def _inputs(h, w, seed=0, planes=3):
    g = np.random.default_rng(seed * 7919 + h * 131 + w)
    return {"random": g.integers(0, 256, (planes, h, w), dtype=np.uint8),
            "binary": (g.integers(0, 2, (planes, h, w)) * 255).astype(np.uint8)}


def _pil_resize(plane_hw, out_h, out_w):
    from PIL import Image
    return np.asarray(Image.fromarray(plane_hw).resize((out_w, out_h), Image.BICUBIC))


def _plain_resize(x, out_h, out_w, **variant):
    """resize of (planes, h, w) to (out_h, out_w) with the restatement's tables and passes, no crop"""
    h, w = x.shape[-2:]
    kh, bh = pp.resample_axis(w, out_w, **variant)
    kv, bv = pp.resample_axis(h, out_h, **variant)
    return pp.resample_pass(pp.resample_pass(x, kh, bh, axis=-1), kv, bv, axis=-2)


# ---- 1. the restatement is Pillow ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", SIZE_PAIRS, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in SIZE_PAIRS])
def test_restatement_equals_pillow(src, dst):
    pytest.importorskip("PIL")
    for kind, x in _inputs(*src).items():
        got = _plain_resize(x, *dst)
        for c in range(x.shape[0]):
            want = _pil_resize(x[c], *dst)
            assert got[c].shape == want.shape
            assert int((got[c] != want).sum()) == 0, (kind, src, dst, c)


def test_pillow_skips_an_axis_of_equal_size():
    """37 x 53 -> 37 x 80 resamples columns only: a bicubic pass over the rows at equal size would change bytes"""
    pytest.importorskip("PIL")
    x = _inputs(37, 53)["random"]
    got = _plain_resize(x, 37, 80)
    assert all(np.array_equal(got[c], _pil_resize(x[c], 37, 80)) for c in range(3))
    k, b = pp.resample_axis(37, 37)
    assert k.shape == (37, 1) and (k == 1 << 22).all() and np.array_equal(b[:, 0], np.arange(37)) and (b[:, 1] == 1).all()


# ---- 2. the library's planner is the restatement -------------------------------------------------------------------------------
def _lib_axis(lib, in_size, out_size, first, count):
    ks = lib.pevit_resize_axis(in_size, out_size, 0, 0, None, None)
    assert ks >= 1
    k = np.full((count, ks), -7, dtype=np.int32)
    b = np.full((count, 2), -7, dtype=np.int32)
    rc = lib.pevit_resize_axis(in_size, out_size, first, count, k.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p))
    assert rc == 0, lib.pevit_last_error()
    return k, b


def _lib_geometry(lib, h, w, n):
    out = [C.c_int() for _ in range(4)]
    assert lib.pevit_resize_geometry(h, w, n, *[C.byref(v) for v in out]) == 0, lib.pevit_last_error()
    return tuple(v.value for v in out)


AXES = sorted({(s[i], d[i]) for s, d in SIZE_PAIRS for i in (0, 1)} |
              {(a, b) for n in GPU_TARGETS + (224,) for h, w in GPU_SOURCES + [(448, 448), (32, 32)]
               for a, b in zip((h, w), pp.resize_geometry(h, w, n)[:2])} | {(37, 37), (1, 5), (5, 1), (4096, 512), (33, 264)})


def test_planner_tables_equal_the_restatement():
    lib = _lib.load()
    for in_size, out_size in AXES:
        k, b = pp.resample_axis(in_size, out_size)
        assert k.shape[1] == pp.axis_ksize(in_size, out_size) == lib.pevit_resize_axis(in_size, out_size, 0, 0, None, None)
        lk, lb = _lib_axis(lib, in_size, out_size, 0, out_size)
        assert np.array_equal(lk, k) and np.array_equal(lb, b), (in_size, out_size)
        first, count = out_size // 3, max(1, out_size // 2)          # a window of rows is the same rows
        wk, wb = _lib_axis(lib, in_size, out_size, first, count)
        assert np.array_equal(wk, k[first:first + count]) and np.array_equal(wb, b[first:first + count])
        pk, pb = pp.resample_axis(in_size, out_size, first, count)
        assert np.array_equal(pk, wk) and np.array_equal(pb, wb)


def test_planner_identity_axis_is_one_tap():
    lib = _lib.load()
    assert lib.pevit_resize_axis(48, 48, 0, 0, None, None) == 1
    k, b = _lib_axis(lib, 48, 48, 5, 9)
    assert (k == 1 << 22).all() and np.array_equal(b[:, 0], np.arange(5, 14)) and (b[:, 1] == 1).all()


def test_planner_geometry_equals_the_restatement():
    lib = _lib.load()
    cases = [(h, w, n) for n in (48, 64, 224) for h, w in GPU_SOURCES + [(448, 448), (500, 300), (300, 500), (1000, 700), (7, 5)]]
    cases += [(48, 53, 48), (48, 55, 48), (53, 48, 48), (55, 48, 48), (48, 54, 48), (48, 52, 48), (48, 49, 48), (48, 51, 48), (224, 224, 224)]
    for h, w, n in cases:
        assert _lib_geometry(lib, h, w, n) == pp.resize_geometry(h, w, n), (h, w, n)
    # Python's round: halves to the even neighbour -- every residue of the difference modulo 4
    assert pp.resize_geometry(48, 53, 48) == (48, 53, 0, 2) and pp.resize_geometry(48, 55, 48) == (48, 55, 0, 4)
    assert pp.resize_geometry(48, 52, 48)[3] == 2 and pp.resize_geometry(48, 54, 48)[3] == 3
    assert pp.resize_geometry(53, 48, 48) == (53, 48, 2, 0) and pp.resize_geometry(55, 48, 48) == (55, 48, 4, 0)
    assert {(pp.resize_geometry(48, 48 + d, 48)[1] - 48) % 4 for d in (4, 5, 6, 7)} == {0, 1, 2, 3}
    assert lib.pevit_resize_geometry(0, 5, 48, *[C.byref(C.c_int()) for _ in range(4)]) != 0


def test_planner_refuses_bad_windows():
    lib = _lib.load()
    k, b = np.zeros((4, 5), np.int32), np.zeros((4, 2), np.int32)
    kp, bp = k.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)
    assert lib.pevit_resize_axis(32, 224, 222, 4, kp, bp) != 0 and b"outside" in lib.pevit_last_error()
    assert lib.pevit_resize_axis(32, 224, -1, 4, kp, bp) != 0
    assert lib.pevit_resize_axis(32, 224, 0, 4, kp, None) != 0
    assert lib.pevit_resize_axis(0, 224, 0, 0, None, None) < 0


# ---- 3. resize + crop + normalise is the reference's transform -----------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(37, 53), (53, 37), (32, 32), (48, 48), (48, 55), (96, 64)])
def test_resize_crop_normalise_equals_the_transform(h, w):
    pytest.importorskip("PIL")
    from PIL import Image
    from pevit_amd.evaluation.clip_load import _Preprocess, _transform
    n = 48
    x = torch.from_numpy(_inputs(h, w, seed=3, planes=6)["random"].reshape(2, 3, h, w))
    got = pp.resize_center_crop_u8(x, n)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 3, n, n)
    mean = torch.tensor(_Preprocess.MEAN).view(1, 3, 1, 1)
    std = torch.tensor(_Preprocess.STD).view(1, 3, 1, 1)
    mine = (got.float() / 255.0 - mean) / std
    for i in range(2):
        want = _transform(n)(Image.fromarray(x[i].permute(1, 2, 0).contiguous().numpy(), "RGB"))
        assert torch.equal(mine[i], want), (h, w, i)


# ---- 4. the bite: a wrong kernel of each kind is seen on the GPU test's list -----------------------------------------------------
def _mutant(x, n, kind):
    h, w = x.shape[-2:]
    nh, nw, top, left = pp.resize_geometry(h, w, n)
    variant = {"a": -0.75} if kind == "a75" else {"normalise": False} if kind == "unnormalised" else {}
    if kind == "crop+1":
        top, left = min(top + 1, nh - n) if nh > n else top, min(left + 1, nw - n) if nw > n else left
        if (top, left) == pp.resize_geometry(h, w, n)[2:]:
            return None                                  # nothing to crop here: this mutant cannot differ
    kh, bh = pp.resample_axis(w, nw, left, n, **variant)
    kv, bv = pp.resample_axis(h, nh, top, n, **variant)

    def one(p, k, b, axis):
        p = np.moveaxis(p, axis, -1).astype(np.int64)
        taps = np.arange(k.shape[1])[None]
        idx = np.minimum(b[:, :1] + taps, p.shape[-1] - 1)
        s = (p[..., idx] * np.where(taps < b[:, 1:2], k, 0)).sum(-1) + (0 if kind == "no-rounding" else 1 << 21)
        if kind == "wrap":
            o = (s >> 22) & 255
        elif kind == "logical-shift":
            o = np.minimum((s & 0xffffffff) >> 22, 255)          # clamps at the top only: a negative sum becomes 255
        else:
            o = np.clip(s >> 22, 0, 255)
        return np.moveaxis(o.astype(np.uint8), -1, axis)
    if kind == "vertical-first":
        return one(one(x, kv, bv, -2), kh, bh, -1)
    return one(one(x, kh, bh, -1), kv, bv, -2)


MUTANTS = ["no-rounding", "vertical-first", "a75", "unnormalised", "wrap", "logical-shift", "crop+1"]


def test_the_unmutated_form_of_the_mutant_code_is_the_restatement():
    for h, w in GPU_SOURCES:
        x = _inputs(h, w)["binary"]
        assert np.array_equal(_mutant(x, 48, "none"), pp.resize_center_crop_u8(x[None], 48)[0])


@pytest.mark.parametrize("kind", MUTANTS)
def test_each_wrong_kernel_is_seen_on_the_gpu_tests_inputs(kind):
    """against Pillow where it is installed (the restatement otherwise, which test 1 holds to Pillow)"""
    seen = []
    for n in GPU_TARGETS:
        for h, w in GPU_SOURCES:
            for name, x in _inputs(h, w).items():
                bad = _mutant(x, n, kind)
                if bad is None:
                    continue
                good = pp.resize_center_crop_u8(x[None], n)[0]
                seen.append(((h, w, n, name), int((bad != good).sum())))
    assert seen and any(d > 0 for _, d in seen), kind
    # the 0 / 255 input shows every mutant at every size that leaves it something to change
    for (h, w, n, name), d in seen:
        resampled = (h, w) != pp.resize_geometry(h, w, n)[:2]
        if name == "binary" and (resampled or kind == "crop+1") and not (kind == "vertical-first" and (h == n or w == n)):
            assert d > 0, (kind, h, w, n)


# ---- 5. exported, declared and typed -------------------------------------------------------------------------------------------
def test_the_three_entries_are_exported_declared_and_typed():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "pevit_hip.h")).read()
    for name in ("pevit_resize_geometry", "pevit_resize_axis", "pevit_resize_u8"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert re.search(r"^int " + name + r"\(", header, re.M), name
    assert len(_lib.SIGNATURES["pevit_resize_u8"][1]) == 14 and len(_lib.SIGNATURES["pevit_resize_axis"][1]) == 6


# ---- 6. pevit_resize_u8 refuses before it launches (so also without a GPU) ------------------------------------------------------
def test_resize_u8_refusals():
    lib = _lib.load()
    p = C.c_void_p(4096)                                  # never dereferenced: every call below is refused on the host

    def call(src=p, planes=3, sh=32, sw=32, dst=p, oh=48, ow=48, kh=p, bh=p, ksh=5, kv=p, bv=p, ksv=5):
        rc = lib.pevit_resize_u8(None, src, planes, sh, sw, dst, oh, ow, kh, bh, ksh, kv, bv, ksv)
        return rc, (lib.pevit_last_error() or b"").decode()

    for null in ("src", "dst", "kh", "bh", "kv", "bv"):
        rc, msg = call(**{null: None})
        assert rc != 0 and "null" in msg, null
    for kw, word in [(dict(ksh=34), "taps"), (dict(ksv=34), "taps"), (dict(ksh=0), "taps"), (dict(ow=257), "output"), (dict(oh=257), "output"),
                     (dict(oh=0), "output"), (dict(ow=0), "output"), (dict(sh=0), "source"), (dict(sw=0), "source"), (dict(sh=4097), "source"),
                     (dict(sw=4097), "source"), (dict(planes=0), "planes")]:
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, msg)


# ---- 7. the loader -------------------------------------------------------------------------------------------------------------
def _archive(tmp_path, h, w, n_train=12, n_test=6, classes=3):
    g = np.random.default_rng(5)
    path = os.path.join(str(tmp_path), "native.npz")
    np.savez(path, train_images=g.integers(0, 256, (n_train, 3, h, w), dtype=np.uint8), train_labels=np.arange(n_train) % classes,
             test_images=g.integers(0, 256, (n_test, 3, h, w), dtype=np.uint8), test_labels=np.arange(n_test) % classes)
    return path


def _config(path, n=48, **dataset):
    from pevit_amd.config import default_config
    cfg = default_config()
    cfg.DATASET.ROOT, cfg.DATASET.DATASET = path, "native"
    cfg.DATASET.NUM_CLASSES, cfg.DATASET.NUM_SAMPLES_PER_CLASS = 3, -1
    cfg.TRAIN.IMAGE_SIZE = [n, n]
    cfg.GPUS = (0,)
    for k, v in dataset.items():
        cfg.DATASET[k] = v
    cfg.DATASET.RESIDENT = False
    return cfg


def test_loader_routes(tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image
    from pevit_amd.evaluation.clip_load import _transform
    from pevit_amd.evaluation.dataloader import construct_dataloader
    path = _archive(tmp_path, 37, 53)
    z = np.load(path)
    test = construct_dataloader(_config(path), test_split_only=True)
    (shape, dtype), _, _ = test.sample_spec()
    assert shape == (3, 37, 53) and dtype == torch.uint8                                   # native size, native bytes
    assert np.array_equal(test.dataset.images.numpy(), z["test_images"])
    host = construct_dataloader(_config(path, RESIZE_ON_HOST=True), test_split_only=True)
    assert host.sample_spec()[0] == ((3, 48, 48), torch.uint8)
    assert torch.equal(host.dataset.images, pp.resize_center_crop_u8(torch.from_numpy(z["test_images"]), 48))
    cfg = _config(path, NORMALIZE_ON_HOST=True)
    cfg.INPUT.MEAN, cfg.INPUT.STD = list(_transform(48).MEAN), list(_transform(48).STD)
    f32 = construct_dataloader(cfg, test_split_only=True)
    assert f32.sample_spec()[0] == ((3, 48, 48), torch.float32)
    for i in range(len(z["test_images"])):
        want = _transform(48)(Image.fromarray(np.ascontiguousarray(z["test_images"][i].transpose(1, 2, 0)), "RGB"))
        assert torch.equal(f32.dataset.images[i], want), i


def test_synthetic_source_size():
    from pevit_amd.evaluation.dataloader import construct_dataloader
    cfg = _config("unused", SYNTHETIC_UINT8=True, SYNTHETIC_SOURCE_SIZE=[32, 40], SYNTHETIC_SIZES=(12, 6))
    cfg.DATASET.DATASET = "synthetic"
    test = construct_dataloader(cfg, test_split_only=True)
    assert test.sample_spec()[0] == ((3, 32, 40), torch.uint8)
    cfg.DATASET.RESIZE_ON_HOST = True
    host = construct_dataloader(cfg, test_split_only=True)
    assert torch.equal(host.dataset.images, pp.resize_center_crop_u8(test.dataset.images, 48))
