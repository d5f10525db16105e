"""The ragged uint8 resize on the GPU (csrc/resize_ragged.hip: pevit_resize_ragged_u8) against the numpy restatement applied image by
image (pevit_amd/preprocess.py: resize_u8), bit for bit: the arithmetic is Pillow's integer arithmetic, so there is no tolerance
anywhere in this file.  tests/test_resize_ragged_host.py holds the restatement's squash mode to Pillow and the pools to the planner.

One ragged set of ten images whose sizes take every branch of the kernel at the targets 48 and 64:
  32 x 32 upscale; 37 x 53 and 53 x 37 unaligned rows, the crop on either axis; 48 x 48 both axes the identity (at 48); 48 x 80 one
  identity axis; 2 x 3 a tiny upscale; 64 x 200 an uneven aspect; 300 x 41, whose squash to 48 needs 2 ceil(2 * 300 / 48) + 1 = 27
  taps, the set's largest ksize_v; 96 x 96 an ordinary downscale; 37 x 53 again, LAST, so that a shared table pair is used twice and
  the last image ends exactly at the end of the pool allocation.
Single launches write into a destination prefilled with a sentinel and fenced by guard bytes on both sides."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from pevit_amd import preprocess as pp

pytestmark = pytest.mark.gpu

SHAPES = [(32, 32), (37, 53), (53, 37), (48, 48), (48, 80), (2, 3), (64, 200), (300, 41), (96, 96), (37, 53)]
TARGETS = (48, 64)
MAX_BATCH = 12
GUARD, SENTINEL = 64, 0xA5
MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


@pytest.fixture(scope="module")
def lib(gpu_required):
    from pevit_amd import _lib
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _set(n, crop, kind="random", shapes=tuple(SHAPES)):
    """(the set on the host, the restatement's (N, 3, n, n) of every image), computed once per case and left unchanged"""
    from pevit_amd import _lib
    g = np.random.default_rng(n + 7 * crop + len(shapes))
    size = int(pp.ragged_offsets(shapes)[-1])
    pool = g.integers(0, 256, size, dtype=np.uint8) if kind == "random" else (g.integers(0, 2, size) * 255).astype(np.uint8)
    r = pp.RaggedImages.build(pool, shapes, n, crop, lib=_lib.load())
    assert r.pre_resized == 0 and r.pool.numel() == size
    return r, pp.resize_ragged_u8(pool, shapes, n, crop)


def _launch(lib, r, index, n, offset=0):
    """one pevit_resize_ragged_u8 on the current stream over the set ``r`` (on the device); ``index``: a list, or None.  Returns
    (dst (B, 3, n, n) on the host, both guards untouched)"""
    from pevit_amd import _lib
    B = len(r) if index is None else len(index)
    idx = None if index is None else torch.tensor(index, dtype=torch.int64, device="cuda")
    size = B * 3 * n * n
    buf = torch.full((GUARD + offset + size + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    a = _lib.PevitResizeRaggedArgs(pool=r.pool.data_ptr(), pool_bytes=r.pool.numel(), desc=r.desc.data_ptr(), k_pool=r.k_pool.data_ptr(),
                                   k_len=r.k_pool.numel(), b_pool=r.b_pool.data_ptr(), b_len=r.b_pool.numel(),
                                   index=None if idx is None else idx.data_ptr(), dst=buf.data_ptr() + GUARD + offset,
                                   n_images=len(r), batch=B, out=n, max_ksize_v=r.max_ksize_v)
    rc = lib.pevit_resize_ragged_u8(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(a))
    assert rc == 0, lib.pevit_last_error()
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    lo, hi = GUARD + offset, GUARD + offset + size
    return out[lo:hi].reshape(B, 3, n, n), bool((out[:lo] == SENTINEL).all() and (out[hi:] == SENTINEL).all())


# ---- 1. single launches ---------------------------------------------------------------------------------------------------------
PERMUTED = [7, 2, 9, 5, 2, 0, 8, 4, 6, 3, 1, 2, 7]                 # every image, 2 three times and 7 twice


@pytest.mark.parametrize("crop", [True, False], ids=["crop", "squash"])
@pytest.mark.parametrize("n", TARGETS)
def test_single_launches_equal_the_restatement(lib, n, crop):
    for kind in ("random", "binary"):
        host, want = _set(n, crop, kind)
        assert int(host.host_desc["offset"][-1]) + 3 * 37 * 53 == host.pool.numel()       # the last image ends with the allocation
        r = host.to("cuda")
        for index in (None, PERMUTED, [7], [5], [9]):                                      # whole set; permuted; one-image batches
            got, fenced = _launch(lib, r, index, n)
            assert fenced, (kind, index)
            assert int((got != want[list(range(len(SHAPES))) if index is None else index]).sum()) == 0, (kind, index)
    assert host.max_ksize_v == {(48, True): 9, (48, False): 27, (64, True): 7, (64, False): 21}[(n, crop)]


@pytest.mark.parametrize("crop", [True, False], ids=["crop", "squash"])
def test_an_odd_destination_address_takes_the_byte_stores(lib, crop):
    host, want = _set(48, crop)
    for offset in (1, 2, 3):
        got, fenced = _launch(lib, host.to("cuda"), PERMUTED, 48, offset=offset)
        assert fenced and int((got != want[PERMUTED]).sum()) == 0, offset


def test_a_target_that_is_no_multiple_of_four_or_of_the_band(lib):
    """out = 50: the last band has 2 rows, the last quad of a row 2 columns, and every store is a byte store"""
    for crop in (True, False):
        host, want = _set(50, crop)
        got, fenced = _launch(lib, host.to("cuda"), PERMUTED, 50)
        assert fenced and int((got != want[PERMUTED]).sum()) == 0, crop


# ---- 2. bits ----------------------------------------------------------------------------------------------------------------------
def test_an_images_bytes_do_not_depend_on_its_neighbours(lib):
    host, want = _set(48, False)
    r = host.to("cuda")
    whole, _ = _launch(lib, r, None, 48)
    for i in range(len(SHAPES)):
        alone, fenced = _launch(lib, r, [i], 48)
        assert fenced and np.array_equal(alone[0], want[i]) and np.array_equal(alone[0], whole[i]), i
    again, _ = _launch(lib, r, PERMUTED[::-1], 48)
    assert np.array_equal(again, whole[PERMUTED[::-1]])


@pytest.mark.parametrize("h,w", [(32, 32), (37, 53), (96, 96)])
def test_a_uniform_ragged_set_gives_the_dense_kernels_bytes(lib, h, w):
    n, B = 48, 5
    host, want = _set(n, True, "random", ((h, w),) * B)
    assert host.k_pool.numel() <= 2 * n * 9 and len(host.keys) <= 2                        # one table pair per axis for the whole set
    ragged, fenced = _launch(lib, host.to("cuda"), None, n)
    nh, nw, top, left = pp.resize_geometry(h, w, n)
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in pp.resample_axis(w, nw, left, n) + pp.resample_axis(h, nh, top, n)]
    src, dst = host.pool.cuda(), torch.empty((3 * B, n, n), dtype=torch.uint8, device="cuda")
    rc = lib.pevit_resize_u8(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(src.data_ptr()), 3 * B, h, w,
                             C.c_void_p(dst.data_ptr()), n, n, C.c_void_p(t[0].data_ptr()), C.c_void_p(t[1].data_ptr()), t[0].shape[1],
                             C.c_void_p(t[2].data_ptr()), C.c_void_p(t[3].data_ptr()), t[2].shape[1])
    assert rc == 0, lib.pevit_last_error()
    torch.cuda.synchronize()
    assert fenced and np.array_equal(ragged, dst.cpu().numpy().reshape(B, 3, n, n)) and np.array_equal(ragged, want)


# ---- 3. the engine ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines(gpu_required):
    """two engines with the same weights and the same adapter / head values: one with the resize on, one without"""
    from conftest import load_tiny_sd
    from pevit_amd.engine import HipEngine, adapter_param_spec
    from pevit_amd.synth import ARCHS, randomize_adapters
    arch, classes = ARCHS["tiny-128"], 10
    sd = {k: v for k, v in load_tiny_sd().items() if k.startswith("visual.")}
    ad = [(n, torch.zeros(s)) for n, s, _ in adapter_param_spec("kadaptation", arch.width, arch.layers)]
    randomize_adapters(ad, seed=3)
    sd.update(dict(ad))
    out = []
    for resize in (True, False):
        eng = HipEngine(arch, "kadaptation", classes, MAX_BATCH)
        eng.load_state_dict(sd)
        g = torch.Generator().manual_seed(11)
        v = eng.param_views()
        with torch.no_grad():
            v["layers.0.weight"].copy_(torch.randn(v["layers.0.weight"].shape, generator=g) * 0.1)
            v["layers.0.bias"].copy_(torch.randn(v["layers.0.bias"].shape, generator=g) * 0.1)
        eng.set_input_normalization(MEAN, STD)
        eng.set_input_resize(resize)
        out.append(eng)
    return out


@pytest.mark.parametrize("crop", [True, False], ids=["crop", "squash"])
def test_engine_calls_on_a_ragged_batch_equal_the_calls_on_the_host_resized_batch(engines, crop):
    on, off = engines
    assert on.arch.resolution == 48
    host, want = _set(48, crop)
    on.set_input_resize(True, center_crop=crop)
    try:
        index = [7, 2, 9, 5, 2, 0, 8, 4, 6, 3, 1]
        batch = host.to("cuda")[index]
        resized = torch.from_numpy(want[index]).cuda()
        labels = torch.randint(0, 10, (len(index),), generator=torch.Generator().manual_seed(3)).cuda()
        assert isinstance(batch, pp.RaggedBatch) and torch.equal(on.resize_u8(batch), resized)
        assert torch.equal(on.predict(batch), off.predict(resized))
        assert torch.equal(on.encode_image(batch), off.encode_image(resized))
        assert torch.equal(on.visual_forward(batch, save=False), off.visual_forward(resized, save=False))
        text = torch.nn.functional.normalize(torch.randn((7, on.arch.embed_dim), generator=torch.Generator().manual_seed(5)), dim=1).cuda()
        for a, b in zip(on.zeroshot(batch, text, return_logits=True), off.zeroshot(resized, text, return_logits=True)):
            assert torch.equal(a, b)
        (l0, s0), (l1, s1) = on.forward_backward(batch, labels), off.forward_backward(resized, labels)
        torch.cuda.synchronize()
        assert torch.equal(l0, l1) and torch.equal(s0, s1)
        assert torch.equal(on.grads, off.grads) and float(on.grads.abs().max()) > 0            # every gradient of the step
        short = host.to("cuda")[[7, 5, 9]]
        assert torch.equal(on.predict(short), off.predict(resized[[0, 3, 2]].contiguous()))     # a shorter batch
    finally:
        on.set_input_resize(True)


def test_dense_native_batches_in_squash_mode(engines):
    on, off = engines
    g = torch.Generator().manual_seed(8)
    native = torch.randint(0, 256, (6, 3, 30, 100), generator=g, dtype=torch.uint8)
    on.set_input_resize(True, center_crop=False)
    try:
        squashed = on.resize_u8(native.cuda()).clone()
        assert torch.equal(squashed.cpu(), pp.resize_u8(native, 48, center_crop=False))
        assert torch.equal(on.predict(native.cuda()), off.predict(squashed))
    finally:
        on.set_input_resize(True)
    assert torch.equal(on.resize_u8(native.cuda()).cpu(), pp.resize_center_crop_u8(native, 48))    # and the crop again, its tables cached apart


def test_refusals(engines):
    from pevit_amd._lib import PevitError
    from pevit_amd.engine import HipEngine
    on, off = engines
    host, _ = _set(48, True)
    batch = host.to("cuda")[[1, 2, 3]]
    labels = torch.zeros(3, dtype=torch.int64, device="cuda")
    with pytest.raises(PevitError, match="ragged"):                                # resize off: a ragged batch cannot be taken
        off.predict(batch)
    with pytest.raises(PevitError, match="ragged"):
        off.forward_backward(batch, labels)
    with pytest.raises(PevitError, match="center_crop"):                           # tables planned for the other mode
        on.predict(_set(48, False)[0].to("cuda")[[1]])
    with pytest.raises(PevitError, match="64 x 64"):                               # ... or for another tower
        on.predict(_set(64, True)[0].to("cuda")[[1]])
    with pytest.raises(PevitError, match=str(on.device)):                          # a batch on the host
        on.predict(host[[1]])
    with pytest.raises(PevitError, match="ensure_batch"):
        on.resize_u8(host.to("cuda")[list(range(10)) + [0, 1, 2]])
    with pytest.raises(PevitError, match="capture_train_step"):
        on._steps, keep = 1, on._steps
        try:
            on.capture_train_step(batch, labels, lr=0.01)
        finally:
            on._steps = keep
    bare = HipEngine(on.arch, "none", 10, MAX_BATCH)
    bare.set_input_resize(True)
    with pytest.raises(PevitError, match="set_input_normalization"):               # uint8 before the constants are known
        bare.predict(batch)


# ---- 4. the probe's feature cache -----------------------------------------------------------------------------------------------------
def test_probe_cache_fill_from_a_ragged_set(engines, tmp_path):
    from conftest import load_tiny_sd
    from test_mirror_api import tiny_config
    from pevit_amd.evaluation import _harness as h, full_model_finetune as fm
    from pevit_amd.evaluation.dataloader import TensorLoader, _Tensors
    ckpt = tmp_path / "tiny.pt"
    torch.save(load_tiny_sd(), ckpt)
    cfg = tiny_config(ckpt, classes=5)
    cfg.TRAIN.FREEZE_IMAGE_BACKBONE = True
    cfg.TEST.BATCH_SIZE_PER_GPU = cfg.TRAIN.BATCH_SIZE_PER_GPU = 8
    h._BACKBONES.clear()
    clf = fm.Classifier(cfg, 0).cuda(0)
    host, want = _set(48, True)
    labels = (torch.arange(len(SHAPES)) % 5).cuda()
    feats = []
    for images in (host.to("cuda"), torch.from_numpy(want).cuda()):
        fm.clear_feature_cache()
        cache = clf.cached(TensorLoader(_Tensors(images, labels), batch_size=4, shuffle=False))
        assert cache is not None and cache.encoded == len(SHAPES)
        feats.append(cache.feats.clone())
    fm.clear_feature_cache(); h._BACKBONES.clear()
    assert torch.equal(feats[0], feats[1]) and float(feats[0].abs().max()) > 0


# ---- 5. the harness: engine resize against DATASET.RESIZE_ON_HOST --------------------------------------------------------------------
def _harness_run(ckpt, host, monkeypatch, dataset):
    from test_mirror_api import tiny_config
    from pevit_amd.evaluation import _harness as h, kadaptation_clip as kc
    from pevit_amd.evaluation import model as mirror
    from pevit_amd.evaluation.dataloader import TensorLoader, construct_dataloader
    cfg = tiny_config(ckpt, classes=5)
    cfg.DATASET.LOADER_BATCH_SIZE = 8
    for k, v in dataset.items():
        cfg.DATASET[k] = v
    cfg.DATASET.RESIZE_ON_HOST = host
    cfg.TRAIN.IMAGE_SIZE = [48, 48]
    cfg.TRAIN.BATCH_SIZE_PER_GPU = cfg.TEST.BATCH_SIZE_PER_GPU = 8
    cfg.TRAIN.LR, cfg.TRAIN.WD, cfg.TRAIN.END_EPOCH = 0.01, 1e-4, 2
    cfg.GPUS = (0,)
    mirror._ENGINES.clear(); h._BACKBONES.clear()
    batches, scored = [], []
    real_iter, real_score = TensorLoader.iter_indices, h._score

    def iter_indices(self):
        for sel in real_iter(self):
            if self.shuffle:
                batches.append(sel.tolist())
            yield sel

    def score(metric, outputs, targets):
        scored.append(torch.cat(outputs).detach().float().cpu())
        return real_score(metric, outputs, targets)
    with monkeypatch.context() as m:
        m.setattr(TensorLoader, "iter_indices", iter_indices)
        m.setattr(h, "_score", score)
        torch.manual_seed(0)
        tr, va, _ = construct_dataloader(cfg)
        images = tr.dataset.dataset.images
        best, info = kc.train_task(tr, va, cfg)
    h._BACKBONES.clear(); mirror._ENGINES.clear()
    return best, batches, scored, images


def _same_run(a, b):
    (b0, batches0, scored0, _), (b1, batches1, scored1, _) = a, b
    assert batches0 == batches1 and len(batches0) == 2 * 4                  # 2 epochs x 30 train rows in batches of 8
    assert len(scored0) == len(scored1) == 4 and all(torch.equal(x, y) for x, y in zip(scored0, scored1))
    assert float(scored0[0].abs().max()) > 0 and b0 == b1


@pytest.mark.parametrize("crop", [True, False], ids=["crop", "squash"])
def test_harness_run_on_a_synthetic_ragged_set_equals_the_host_resized_run(gpu_required, tmp_path, monkeypatch, crop):
    from conftest import load_tiny_sd
    ckpt = tmp_path / "tiny.pt"
    torch.save(load_tiny_sd(), ckpt)
    dataset = dict(DATASET="synthetic", SYNTHETIC_SIZES=(40, 10), SYNTHETIC_RAGGED=True, SYNTHETIC_SOURCE_RANGE=[20, 90], CENTER_CROP=crop)
    on_host = _harness_run(ckpt, True, monkeypatch, dataset)
    on_engine = _harness_run(ckpt, False, monkeypatch, dataset)
    assert isinstance(on_host[3], torch.Tensor) and tuple(on_host[3].shape[1:]) == (3, 48, 48)
    ragged = on_engine[3]
    assert isinstance(ragged, pp.RaggedImages) and ragged.device.type == "cuda" and ragged.center_crop == crop and len(ragged) == 40
    assert torch.equal(ragged.resize_on_host(), on_host[3].cpu())           # the same pictures went into both runs
    _same_run(on_host, on_engine)


def test_harness_run_without_the_centre_crop_on_a_dense_native_archive(gpu_required, tmp_path, monkeypatch):
    from conftest import load_tiny_sd
    ckpt = tmp_path / "tiny.pt"
    torch.save(load_tiny_sd(), ckpt)
    g = np.random.default_rng(4)
    np.savez(os.path.join(str(tmp_path), "wide.npz"), train_images=g.integers(0, 256, (40, 3, 30, 100), dtype=np.uint8),
             train_labels=np.arange(40) % 5, test_images=g.integers(0, 256, (10, 3, 30, 100), dtype=np.uint8), test_labels=np.arange(10) % 5)
    z = np.load(os.path.join(str(tmp_path), "wide.npz"))
    dataset = dict(DATASET="wide", ROOT=str(tmp_path), CENTER_CROP=False)
    on_host = _harness_run(ckpt, True, monkeypatch, dataset)
    on_engine = _harness_run(ckpt, False, monkeypatch, dataset)
    assert tuple(on_engine[3].shape[1:]) == (3, 30, 100) and on_engine[3].device.type == "cuda"        # the native set stays native
    assert torch.equal(on_host[3].cpu(), pp.resize_u8(torch.from_numpy(z["train_images"]), 48, center_crop=False))
    _same_run(on_host, on_engine)
    cropped = _harness_run(ckpt, True, monkeypatch, dict(dataset, CENTER_CROP=True))
    assert not all(torch.equal(x, y) for x, y in zip(cropped[2], on_host[2]))                           # the key has an effect
