"""Ragged uint8 sets -- one size per image -- and the squash mode of DATASET.CENTER_CROP False, without a GPU.

* ``preprocess.resize_u8(..., center_crop=False)`` is Pillow's ``resize((n, n), BICUBIC)``, byte for byte.
* ``preprocess.RaggedImages.build``: every image's tables are ``resample_axis`` of its axis keys, images that share a key share its
  rows, offsets are int64, images outside the kernel's range are stored pre-resized; the loader falls back to the dense
  host-resized tensor where the set cannot stay ragged.
* ``pevit_resize_ragged_check`` refuses each kind of bad descriptor with a message that names it, and ``pevit_resize_ragged_u8``
  refuses null pointers and ``batch < 1`` before any launch (so also here, where there is no GPU to launch on).
* the loader routes."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from pevit_amd import _lib
from pevit_amd import preprocess as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (h, w): every branch of the kernel at targets 48 and 64 (tests/test_gpu_resize_ragged.py uses the same set)
SHAPES = [(32, 32), (37, 53), (53, 37), (48, 48), (48, 80), (2, 3), (64, 200), (300, 41), (96, 96), (37, 53)]


def _pool(shapes, seed=0, kind="random"):
    g = np.random.default_rng(seed)
    n = int(pp.ragged_offsets(shapes)[-1])
    return g.integers(0, 256, n, dtype=np.uint8) if kind == "random" else (g.integers(0, 2, n) * 255).astype(np.uint8)


# ---- 1. squash mode against Pillow ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [48, 64])
@pytest.mark.parametrize("h,w", [(75, 248), (248, 75), (90, 90), (48, 48), (64, 64), (30, 100), (2, 3), (300, 41)],
                         ids=lambda v: str(v))
def test_squash_mode_is_pillows_resize(h, w, n):
    pytest.importorskip("PIL")
    from PIL import Image
    g = np.random.default_rng(h * 1009 + w * 17 + n)
    for x in (g.integers(0, 256, (3, h, w), dtype=np.uint8), (g.integers(0, 2, (3, h, w)) * 255).astype(np.uint8)):
        got = pp.resize_u8(x[None], n, center_crop=False)[0]
        want = np.stack([np.asarray(Image.fromarray(x[c]).resize((n, n), Image.BICUBIC)) for c in range(3)])
        assert got.shape == (3, n, n) and int((got != want).sum()) == 0
        t = pp.resize_u8(torch.from_numpy(x[None].copy()), n, center_crop=False)
        assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy()[0], want)


def test_resize_u8_with_the_crop_is_resize_center_crop_u8():
    x = np.random.default_rng(1).integers(0, 256, (2, 3, 37, 53), dtype=np.uint8)
    assert np.array_equal(pp.resize_u8(x, 48), pp.resize_center_crop_u8(x, 48))
    assert np.array_equal(pp.resize_u8(x, 48, center_crop=True), pp.resize_center_crop_u8(x, 48))
    assert not np.array_equal(pp.resize_u8(x, 48, center_crop=False), pp.resize_center_crop_u8(x, 48))


def test_the_axis_keys_of_both_modes():
    assert pp.axis_keys(37, 53, 48, True) == ((53, 68, 10), (37, 48, 0))
    assert pp.axis_keys(37, 53, 48, False) == ((53, 48, 0), (37, 48, 0))
    assert pp.axis_keys(375, 1242, 224, False) == ((1242, 224, 0), (375, 224, 0))
    assert pp.axis_ksize(1242, 224) == 25 and pp.in_kernel_range(375, 1242, 224, False)      # kitti's squash is inside the kernel's 33
    assert pp.axis_ksize(300, 48) == 27 and pp.in_kernel_range(300, 41, 48, False)
    assert not pp.in_kernel_range(4097, 100, 48, True) and not pp.in_kernel_range(500, 500, 48, True)    # a side; 10.4x: 43 taps


# ---- 2. pool building ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crop", [True, False], ids=["crop", "squash"])
@pytest.mark.parametrize("n", [48, 64])
def test_pool_building(n, crop):
    pool = _pool(SHAPES)
    r = pp.RaggedImages.build(pool, SHAPES, n, crop, lib=_lib.load())
    assert len(r) == len(SHAPES) and r.pre_resized == 0 and r.out == n and r.center_crop == crop
    assert r.pool.dtype == torch.uint8 and r.pool.dim() == 1 and np.array_equal(r.pool.numpy(), pool)      # the archive's bytes
    d = r.host_desc
    assert d.dtype == pp.RAGGED_DESC and d["offset"].dtype == np.int64
    assert np.array_equal(d["offset"], pp.ragged_offsets(SHAPES)[:-1]) and pp.ragged_offsets(SHAPES).dtype == np.int64
    assert r.desc.dtype == torch.int32 and tuple(r.desc.shape) == (len(SHAPES), 10)
    assert r.desc.numpy().tobytes() == d.tobytes()                                             # the struct's bytes, as uploaded
    k_pool, b_pool = r.k_pool.numpy(), r.b_pool.numpy()
    assert k_pool.dtype == b_pool.dtype == np.int32
    for i, (h, w) in enumerate(SHAPES):
        assert (int(d["h"][i]), int(d["w"][i])) == (h, w)
        for axis, key in zip("hv", pp.axis_keys(h, w, n, crop)):
            k, b = pp.resample_axis(key[0], key[1], key[2], n)                                 # the planner's oracle
            ko, bo, ks = int(d[f"k{axis}_off"][i]), int(d[f"b{axis}_off"][i]), int(d[f"ksize_{axis}"][i])
            assert ks == k.shape[1] == pp.axis_ksize(key[0], key[1])
            assert np.array_equal(k_pool[ko:ko + n * ks].reshape(n, ks), k), (i, axis)
            assert np.array_equal(b_pool[bo:bo + 2 * n].reshape(n, 2), b), (i, axis)
    # images that share a key share its rows: 37 x 53 twice, and its axes again in 53 x 37; the pool holds each key once
    assert d[1][["kh_off", "bh_off", "kv_off", "bv_off"]] == d[9][["kh_off", "bh_off", "kv_off", "bv_off"]]
    keys = {key for h, w in SHAPES for key in pp.axis_keys(h, w, n, crop)}
    assert set(r.keys) == keys
    assert k_pool.size == sum(n * pp.axis_ksize(i, o) for i, o, _ in keys) and b_pool.size == 2 * n * len(keys)
    assert r.table_bytes == pp.ragged_table_bytes(SHAPES, n, crop)
    assert r.max_ksize_v == max(pp.axis_ksize(h, pp.axis_keys(h, w, n, crop)[1][1]) for h, w in SHAPES)
    if not crop and n == 48:
        assert r.max_ksize_v == 27                   # 300 -> 48: 2 ceil(2 * 300 / 48) + 1


def test_indexing_copies_no_pixel():
    r = pp.RaggedImages.build(_pool(SHAPES), SHAPES, 48)
    for index in (torch.tensor([3, 1, 1, 8]), np.array([3, 1, 1, 8]), [3, 1, 1, 8]):
        b = r[index]
        assert isinstance(b, pp.RaggedBatch) and b.index.dtype == torch.int64 and b.index.tolist() == [3, 1, 1, 8]
        assert b.pool.data_ptr() == r.pool.data_ptr() and b.desc.data_ptr() == r.desc.data_ptr()
        assert b.k_pool.data_ptr() == r.k_pool.data_ptr() and b.b_pool.data_ptr() == r.b_pool.data_ptr()
        assert len(b) == 4 and b.shape == (4, 3, 0, 0) and b.dtype == torch.uint8 and b.dim() == 4 and b.contiguous() is b
    assert r.to("cpu") is r and r[[0]].to("cpu").images is r
    sub = r.subset(np.array([9, 2, 5]))
    assert len(sub) == 3 and sub.pool.data_ptr() == r.pool.data_ptr() and sub.k_pool.data_ptr() == r.k_pool.data_ptr()
    assert sub.host_desc.tobytes() == r.host_desc[[9, 2, 5]].tobytes()
    assert torch.equal(sub.image(0), r.image(9)) and tuple(sub.image(1).shape) == (3, 53, 37)
    want = torch.cat([pp.resize_u8(r.image(i)[None].contiguous(), 48) for i in (3, 1, 1, 8)])
    assert torch.equal(r[[3, 1, 1, 8]].resize_on_host(), want)
    assert np.array_equal(pp.resize_ragged_u8(r.pool.numpy(), SHAPES, 48)[[3, 1, 1, 8]], want.numpy())


@pytest.mark.parametrize("crop", [True, False], ids=["crop", "squash"])
def test_images_outside_the_kernels_range_are_stored_resized(crop):
    shapes = [(40, 40), (4100, 8), (48, 48), (450, 450), (20, 30)]                       # a side above 4096; 9.4x: 39 taps
    pool = _pool(shapes, seed=3)
    off = pp.ragged_offsets(shapes)
    r = pp.RaggedImages.build(pool, shapes, 48, crop, lib=_lib.load())
    assert r.pre_resized == 2
    assert [(int(h), int(w)) for h, w in zip(r.host_desc["h"], r.host_desc["w"])] == [(40, 40), (48, 48), (48, 48), (48, 48), (20, 30)]
    assert np.array_equal(r.host_desc["offset"], pp.ragged_offsets([(40, 40), (48, 48), (48, 48), (48, 48), (20, 30)])[:-1])
    for i in (1, 3):
        want = pp.resize_u8(pp.ragged_image(pool, shapes, off, i)[None], 48, crop)[0]
        assert np.array_equal(r.image(i).numpy(), want)
        assert int(r.host_desc["ksize_h"][i]) == int(r.host_desc["ksize_v"][i]) == 1       # both axes: the one-tap identity
        assert r.host_desc[i][["kh_off", "bh_off", "kv_off", "bv_off"]] == r.host_desc[2][["kh_off", "bh_off", "kv_off", "bv_off"]]
    for i in (0, 2, 4):
        assert np.array_equal(r.image(i).numpy(), pp.ragged_image(pool, shapes, off, i))
    assert torch.equal(r.resize_on_host(), torch.from_numpy(pp.resize_ragged_u8(pool, shapes, 48, crop)))


def test_build_refuses_what_does_not_describe_the_pool():
    with pytest.raises(ValueError, match="bytes"):
        pp.RaggedImages.build(_pool(SHAPES)[:-1], SHAPES, 48)
    with pytest.raises(ValueError, match="target"):
        pp.RaggedImages.build(_pool(SHAPES), SHAPES, 257)
    with pytest.raises(ValueError, match="side"):
        pp.RaggedImages.build(np.zeros(0, dtype=np.uint8), [(0, 4)], 48)


# ---- 3. pevit_resize_ragged_check ----------------------------------------------------------------------------------------------
def _check(lib, desc, pool_bytes, k_len, b_len, out=48):
    rc = lib.pevit_resize_ragged_check(C.c_void_p(desc.ctypes.data), len(desc), pool_bytes, k_len, b_len, out)
    return rc, (lib.pevit_last_error() or b"").decode()


def test_check_refuses_each_bad_descriptor_by_name():
    lib = _lib.load()
    r = pp.RaggedImages.build(_pool(SHAPES), SHAPES, 48, lib=lib)
    sizes = (r.pool.numel(), r.k_pool.numel(), r.b_pool.numel())
    good = r.host_desc
    assert _check(lib, good, *sizes)[0] == 0
    last = len(good) - 1
    assert int(good["offset"][last]) + 3 * 37 * 53 == sizes[0]                              # the last image ends with the pool
    cases = [("offset", last, int(good["offset"][last]) + 1, "past the pool"), ("offset", 0, -1, "past the pool"),
             ("h", last, 38, "past the pool"),
             ("h", 2, 0, "sides"), ("w", 2, 0, "sides"), ("h", 2, 4097, "sides"), ("w", 2, 4097, "sides"),
             ("ksize_h", 4, 0, "ksize"), ("ksize_v", 4, 0, "ksize"), ("ksize_h", 4, 34, "ksize"), ("ksize_v", 4, 34, "ksize"),
             ("kh_off", 5, sizes[1] - 48 * 5 + 1, "table range"), ("kv_off", 5, -1, "table range"),
             ("bh_off", 5, sizes[2] - 2 * 48 + 1, "table range"), ("bv_off", 5, -4, "table range"), ("ksize_v", 8, 33, "table range")]
    for field, i, value, word in cases:
        bad = good.copy()
        bad[field][i] = value
        rc, msg = _check(lib, bad, *sizes)
        assert rc != 0 and word in msg and f"image {i}" in msg, (field, i, value, msg)
    rc, msg = _check(lib, good, *sizes, out=257)
    assert rc != 0 and "out 257" in msg
    rc, msg = _check(lib, good, *sizes, out=0)
    assert rc != 0 and "out 0" in msg
    rc = lib.pevit_resize_ragged_check(None, 3, *sizes, 48)
    assert rc != 0 and b"null" in lib.pevit_last_error()
    rc = lib.pevit_resize_ragged_check(C.c_void_p(good.ctypes.data), 0, *sizes, 48)
    assert rc != 0 and b"0 images" in lib.pevit_last_error()
    with pytest.raises(ValueError, match="past the pool"):                                   # build() runs the check
        class _Short:                                                                        # the library, with a pool one byte short
            def __getattr__(self, name):
                return getattr(lib, name)

            def pevit_resize_ragged_check(self, d, n, pool_bytes, k_len, b_len, out):
                return lib.pevit_resize_ragged_check(d, n, pool_bytes - 1, k_len, b_len, out)
        pp.RaggedImages.build(_pool(SHAPES), SHAPES, 48, lib=_Short())


# ---- 4. pevit_resize_ragged_u8 refuses before it launches ------------------------------------------------------------------------
def test_resize_ragged_u8_refusals():
    lib = _lib.load()
    p = 4096                                              # never dereferenced: every call below is refused on the host

    def call(**kw):
        a = dict(pool=p, pool_bytes=1 << 20, desc=p, k_pool=p, k_len=1 << 16, b_pool=p, b_len=1 << 12, index=p, dst=p, n_images=4,
                 batch=2, out=48, max_ksize_v=9)
        a.update(kw)
        args = _lib.PevitResizeRaggedArgs(**a)
        rc = lib.pevit_resize_ragged_u8(None, C.byref(args))
        return rc, (lib.pevit_last_error() or b"").decode()

    for null in ("pool", "desc", "k_pool", "b_pool", "dst"):
        rc, msg = call(**{null: None})
        assert rc != 0 and "null" in msg, null
    rc = lib.pevit_resize_ragged_u8(None, None)
    assert rc != 0 and b"null" in lib.pevit_last_error()
    for kw, word in [(dict(batch=0), "batch 0"), (dict(batch=-3), "batch -3"), (dict(n_images=0), "0 images"), (dict(out=257), "out 257"),
                     (dict(out=0), "out 0"), (dict(max_ksize_v=34), "ksize_v 34"), (dict(max_ksize_v=0), "ksize_v 0"),
                     (dict(pool_bytes=2), "pools"), (dict(k_len=47), "pools"), (dict(b_len=95), "pools")]:
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, msg)


# ---- 5. exported, declared and typed ---------------------------------------------------------------------------------------------
def test_the_two_entries_are_exported_declared_and_typed():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "pevit_hip.h")).read()
    for name in ("pevit_resize_ragged_check", "pevit_resize_ragged_u8"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        assert re.search(r"^int " + name + r"\(", header, re.M), name
    assert C.sizeof(_lib.PevitResizeRaggedDesc) == pp.RAGGED_DESC.itemsize == 40
    for (name, _), (np_name, (np_type, np_off)) in zip(_lib.PevitResizeRaggedDesc._fields_, sorted(pp.RAGGED_DESC.fields.items(), key=lambda f: f[1][1])):
        assert name == np_name and getattr(_lib.PevitResizeRaggedDesc, name).offset == np_off
    for field in ("int64_t offset", "int32_t h, w", "kh_off, bh_off, ksize_h", "kv_off, bv_off, ksize_v", "const uint8_t* pool",
                  "const int64_t* index", "max_ksize_v"):
        assert field in header, field
    assert [n for n, _ in _lib.PevitResizeRaggedArgs._fields_] == ["pool", "pool_bytes", "desc", "k_pool", "k_len", "b_pool", "b_len", "index",
                                                                   "dst", "n_images", "batch", "out", "max_ksize_v"]
    assert "resize_ragged.hip" in open(os.path.join(ROOT, "pevit_amd", "csrc", "Makefile")).read()


# ---- 6. the loader -----------------------------------------------------------------------------------------------------------------
TRAIN_SHAPES = [(37, 53), (48, 48), (20, 64), (53, 37), (64, 64), (33, 90), (37, 53), (48, 80), (96, 96), (25, 25), (40, 31), (31, 40)]
TEST_SHAPES = [(32, 32), (75, 40), (48, 48), (30, 100), (2, 3), (64, 50)]


def _archive(tmp_path, train_shapes=TRAIN_SHAPES, test_shapes=TEST_SHAPES, classes=3):
    path = os.path.join(str(tmp_path), "ragged.npz")
    np.savez(path, train_images=_pool(train_shapes, 5), train_shapes=np.asarray(train_shapes), train_labels=np.arange(len(train_shapes)) % classes,
             test_images=_pool(test_shapes, 6), test_shapes=np.asarray(test_shapes), test_labels=np.arange(len(test_shapes)) % classes)
    return path


def _config(path, n=48, **dataset):
    from pevit_amd.config import default_config
    cfg = default_config()
    cfg.DATASET.ROOT, cfg.DATASET.DATASET = path, "ragged"
    cfg.DATASET.NUM_CLASSES, cfg.DATASET.NUM_SAMPLES_PER_CLASS = 3, -1
    cfg.TRAIN.IMAGE_SIZE = [n, n]
    cfg.GPUS = (0,)
    for k, v in dataset.items():
        cfg.DATASET[k] = v
    return cfg


@pytest.fixture
def resident(monkeypatch):
    """the loader as it decides on a machine with a GPU -- the set counts as resident -- with its tensors kept on the host, GPU or not"""
    from pevit_amd.evaluation import dataloader
    monkeypatch.setattr(dataloader, "_ragged_stays", lambda config, dev: not config.DATASET.get("RESIZE_ON_HOST", False)
                        and not config.DATASET.get("NORMALIZE_ON_HOST", False) and config.DATASET.get("RESIDENT", True))
    monkeypatch.setattr(dataloader, "_resident_device", lambda config, nbytes, limit=0: torch.device("cpu"))


@pytest.mark.parametrize("crop", [True, False], ids=["crop", "squash"])
def test_a_ragged_archive_stays_ragged(tmp_path, resident, crop):
    from pevit_amd.evaluation.dataloader import construct_dataloader
    path = _archive(tmp_path)
    z = np.load(path)
    test = construct_dataloader(_config(path, CENTER_CROP=crop), test_split_only=True)
    images = test.dataset.images
    assert isinstance(images, pp.RaggedImages) and images.center_crop == crop and images.out == 48       # CENTER_CROP reaches the geometry
    assert np.array_equal(images.pool.numpy(), z["test_images"])                                         # the archive's bytes
    assert test.sample_spec()[0] == ((3, 0, 0), torch.uint8)
    for i, (h, w) in enumerate(TEST_SHAPES):
        keys = pp.axis_keys(h, w, 48, crop)
        assert (int(images.host_desc["ksize_h"][i]), int(images.host_desc["ksize_v"][i])) == tuple(pp.axis_ksize(k[0], k[1]) for k in keys)
    batches = list(test)
    assert len(batches) == 1 and isinstance(batches[0][0], pp.RaggedBatch) and batches[0][0].index.tolist() == list(range(6))
    assert batches[0][0].pool.data_ptr() == images.pool.data_ptr() and batches[0][1].tolist() == [0, 1, 2, 0, 1, 2]
    want = np.stack([pp.resize_u8(pp.ragged_image(z["test_images"], TEST_SHAPES, pp.ragged_offsets(TEST_SHAPES), i)[None], 48, crop)[0]
                     for i in range(6)])
    assert np.array_equal(batches[0][0].resize_on_host().numpy(), want)


def test_the_few_shot_subset_and_the_split_index_the_pool(tmp_path, resident):
    from pevit_amd.evaluation._harness import merge_trainval_loader
    from pevit_amd.evaluation.dataloader import construct_dataloader
    path = _archive(tmp_path)
    z = np.load(path)
    tr, va, te = construct_dataloader(_config(path))
    full = tr.dataset.dataset
    assert full is va.dataset.dataset and isinstance(full.images, pp.RaggedImages) and len(full) == 12
    assert np.array_equal(full.images.pool.numpy(), z["train_images"]) and len(tr.dataset) + len(va.dataset) == 12
    assert sorted(tr.dataset.indices + va.dataset.indices) == list(range(12))
    seen = []
    for x, y in va:
        assert isinstance(x, pp.RaggedBatch) and x.pool.data_ptr() == full.images.pool.data_ptr()
        seen += x.index.tolist()
        assert y.tolist() == [i % 3 for i in x.index.tolist()]
    assert seen == va.dataset.indices
    merged = merge_trainval_loader(tr, va)
    assert sorted(i for x, _ in merged for i in x.index.tolist()) == list(range(12))
    cfg = _config(path)
    cfg.DATASET.NUM_SAMPLES_PER_CLASS = 2
    tr2, va2, _ = construct_dataloader(cfg)
    sub = tr2.dataset.dataset
    assert len(sub) == 6 and sub.images.pool.data_ptr() != 0 and np.array_equal(sub.images.pool.numpy(), z["train_images"])     # the whole pool, indexed
    from pevit_amd.evaluation.dataloader import few_shot_subset
    keep = few_shot_subset(np.arange(12) % 3, 2, 0)
    assert sub.images.host_desc.tobytes() == pp.RaggedImages.build(z["train_images"], TRAIN_SHAPES, 48).host_desc[keep].tobytes()
    assert sub.labels.tolist() == [int(i) % 3 for i in keep]


@pytest.mark.parametrize("crop", [True, False], ids=["crop", "squash"])
@pytest.mark.parametrize("why", ["RESIZE_ON_HOST", "not-resident", "cap", "no-gpu"])
def test_a_set_that_cannot_stay_ragged_is_resized_on_the_host(tmp_path, monkeypatch, why, crop):
    from pevit_amd.evaluation import dataloader
    path = _archive(tmp_path)
    z = np.load(path)
    kw = {"RESIZE_ON_HOST": dict(RESIZE_ON_HOST=True), "not-resident": dict(RESIDENT=False), "cap": dict(RAGGED_TABLE_BYTES=4096),
          "no-gpu": {}}[why]
    monkeypatch.setattr(dataloader, "_resident_device", lambda config, nbytes, limit=0: torch.device("cpu"))     # tensors on the host, GPU or not
    if why != "no-gpu":                              # "no-gpu": the loader's own rule for a set whose device is the CPU
        monkeypatch.setattr(dataloader, "_ragged_stays", lambda config, dev: not config.DATASET.get("RESIZE_ON_HOST", False)
                            and config.DATASET.get("RESIDENT", True))
    test = dataloader.construct_dataloader(_config(path, CENTER_CROP=crop, **kw), test_split_only=True)
    assert isinstance(test.dataset.images, torch.Tensor) and test.sample_spec()[0] == ((3, 48, 48), torch.uint8)
    off = pp.ragged_offsets(TEST_SHAPES)
    for i in range(len(TEST_SHAPES)):
        want = pp.resize_u8(pp.ragged_image(z["test_images"], TEST_SHAPES, off, i)[None], 48, crop)[0]
        assert np.array_equal(test.dataset.images[i].numpy(), want), i
    if why == "cap":
        assert pp.ragged_table_bytes(TEST_SHAPES, 48, crop) > 4096


def test_out_of_range_images_reach_the_loader_resized(tmp_path, resident):
    from pevit_amd.evaluation.dataloader import construct_dataloader
    shapes = [(30, 30), (500, 48), (48, 48), (20, 20), (10, 10), (60, 60)]                 # 500 -> 48 with the crop: 500 x 48, in range
    path = _archive(tmp_path, test_shapes=shapes)
    images = construct_dataloader(_config(path, CENTER_CROP=False), test_split_only=True).dataset.images
    assert images.pre_resized == 1 and (int(images.host_desc["h"][1]), int(images.host_desc["w"][1])) == (48, 48)     # 10.4x: 43 taps
    z = np.load(path)
    want = pp.resize_u8(pp.ragged_image(z["test_images"], shapes, pp.ragged_offsets(shapes), 1)[None], 48, False)[0]
    assert np.array_equal(images.image(1).numpy(), want)
    assert construct_dataloader(_config(path), test_split_only=True).dataset.images.pre_resized == 0


def test_a_dense_archive_takes_the_old_route_and_center_crop_reaches_its_host_resize(tmp_path):
    from pevit_amd.evaluation.dataloader import construct_dataloader
    g = np.random.default_rng(5)
    path = os.path.join(str(tmp_path), "ragged.npz")
    np.savez(path, train_images=g.integers(0, 256, (6, 3, 30, 100), dtype=np.uint8), train_labels=np.arange(6) % 3,
             test_images=g.integers(0, 256, (6, 3, 30, 100), dtype=np.uint8), test_labels=np.arange(6) % 3)
    z = np.load(path)
    native = construct_dataloader(_config(path, RESIDENT=False), test_split_only=True)
    assert isinstance(native.dataset.images, torch.Tensor) and native.sample_spec()[0] == ((3, 30, 100), torch.uint8)
    assert np.array_equal(native.dataset.images.numpy(), z["test_images"])
    crop = construct_dataloader(_config(path, RESIDENT=False, RESIZE_ON_HOST=True), test_split_only=True)
    assert torch.equal(crop.dataset.images, pp.resize_center_crop_u8(torch.from_numpy(z["test_images"]), 48))
    squash = construct_dataloader(_config(path, RESIDENT=False, RESIZE_ON_HOST=True, CENTER_CROP=False), test_split_only=True)
    assert torch.equal(squash.dataset.images, pp.resize_u8(torch.from_numpy(z["test_images"]), 48, center_crop=False))
    assert not torch.equal(squash.dataset.images, crop.dataset.images)


def test_synthetic_ragged_sets(resident):
    from pevit_amd.evaluation.dataloader import construct_dataloader
    cfg = _config("unused", SYNTHETIC_RAGGED=True, SYNTHETIC_SOURCE_RANGE=[20, 70], SYNTHETIC_SIZES=(12, 6))
    cfg.DATASET.DATASET = "synthetic"
    a, b = (construct_dataloader(cfg, test_split_only=True).dataset.images for _ in range(2))
    assert isinstance(a, pp.RaggedImages) and len(a) == 6 and torch.equal(a.pool, b.pool) and a.host_desc.tobytes() == b.host_desc.tobytes()
    sides = np.concatenate([a.host_desc["h"], a.host_desc["w"]])
    assert sides.min() >= 20 and sides.max() <= 70 and len(set(zip(a.host_desc["h"].tolist(), a.host_desc["w"].tolist()))) > 1
    cfg.DATASET.RESIZE_ON_HOST = True
    host = construct_dataloader(cfg, test_split_only=True)
    assert torch.equal(host.dataset.images, a.resize_on_host())


def test_the_mirror_and_the_classifier_pass_the_mode_on():
    import inspect
    from pevit_amd.engine import HipEngine
    from pevit_amd.evaluation import _harness, model
    for fn in (HipEngine.set_input_resize, model.VisionTransformer.set_input_resize):
        p = inspect.signature(fn).parameters
        assert list(p)[1:] == ["on", "center_crop"] and p["center_crop"].default is True
    src = inspect.getsource(_harness.ClassifierBase.__init__)
    assert re.search(r"set_input_resize\(True, .*CENTER_CROP", src)
