"""The uint8 resize on the GPU (csrc/resize.hip: pevit_resize_u8) against the numpy restatement (pevit_amd/preprocess.py), bit for bit:
Pillow's 8-bit bicubic resize is integer arithmetic, so there is no tolerance anywhere in this file.  tests/test_resize_host.py holds
the restatement to Pillow and shows that a wrong kernel of each kind (no rounding term, vertical pass first, another bicubic
parameter, taps not normalised, wrap or logical shift instead of the clamp, a shifted crop window) differs on the inputs used here.

Single launches write into a destination prefilled with a sentinel and fenced by guard bytes on both sides; the source tensor is
allocated at exactly planes * h * w bytes."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from pevit_amd import preprocess as pp

pytestmark = pytest.mark.gpu

SOURCES = [(8, 8), (32, 32), (37, 53), (53, 37), (48, 55), (96, 96), (384, 384)]       # (h, w); 384 -> 48 is the 8x cap: 33 taps
TARGETS = (48, 64)
MAX_BATCH = 8
GUARD, SENTINEL = 64, 0xA5


@pytest.fixture(scope="module")
def lib(gpu_required):
    from pevit_amd import _lib
    return _lib.load()


@functools.lru_cache(maxsize=None)
def _case(h, w, n, planes, kind):
    """(source (planes, h, w) uint8, the restatement's (planes, n, n)), computed once per case"""
    g = np.random.default_rng(h * 1009 + w * 17 + n + planes)
    x = g.integers(0, 256, (planes, h, w), dtype=np.uint8) if kind == "random" else (g.integers(0, 2, (planes, h, w)) * 255).astype(np.uint8)
    return x, pp.resize_center_crop_u8(x[None], n)[0]


def _tables(h, w, n):
    nh, nw, top, left = pp.resize_geometry(h, w, n)
    return pp.resample_axis(w, nw, left, n) + pp.resample_axis(h, nh, top, n)


def _launch(lib, x, out_h, out_w, kh, bh, kv, bv, offset=0):
    """one pevit_resize_u8 on the current stream; returns (dst (planes, out_h, out_w) on the host, both guards untouched)"""
    planes, h, w = x.shape
    src = torch.from_numpy(np.ascontiguousarray(x)).cuda()                       # exactly planes * h * w bytes
    dev = [torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in (kh, bh, kv, bv)]
    n = planes * out_h * out_w
    buf = torch.full((GUARD + offset + n + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    rc = lib.pevit_resize_u8(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(src.data_ptr()), planes, h, w,
                             C.c_void_p(buf.data_ptr() + GUARD + offset), out_h, out_w, C.c_void_p(dev[0].data_ptr()),
                             C.c_void_p(dev[1].data_ptr()), kh.shape[1], C.c_void_p(dev[2].data_ptr()), C.c_void_p(dev[3].data_ptr()),
                             kv.shape[1])
    assert rc == 0, lib.pevit_last_error()
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    lo, hi = GUARD + offset, GUARD + offset + n
    return out[lo:hi].reshape(planes, out_h, out_w), bool((out[:lo] == SENTINEL).all() and (out[hi:] == SENTINEL).all())


# ---- 1. single launches ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", TARGETS)
@pytest.mark.parametrize("h,w", SOURCES, ids=[f"{h}x{w}" for h, w in SOURCES])
def test_single_launches_equal_the_restatement(lib, h, w, n):
    for planes in (3, 9, 3 * MAX_BATCH):
        for kind in ("random", "binary"):
            x, want = _case(h, w, n, planes, kind)
            got, fenced = _launch(lib, x, n, n, *_tables(h, w, n))
            assert fenced, (planes, kind)
            assert int((got != want).sum()) == 0, (planes, kind)


@pytest.mark.parametrize("h,w", [(32, 32), (448, 448)], ids=["32", "448"])
def test_the_production_target_224(lib, h, w):
    x, want = _case(h, w, 224, 3, "random")
    got, fenced = _launch(lib, x, 224, 224, *_tables(h, w, 224))
    assert fenced and int((got != want).sum()) == 0


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "odd-address"])
@pytest.mark.parametrize("out_h,out_w", [(40, 23), (7, 64), (17, 1)])
def test_windows_that_are_no_multiple_of_the_band_or_of_four_columns(lib, out_h, out_w, offset):
    """tables of the caller's own: a window of out_h rows and out_w columns of the 53 x 37 -> 91 x 64 resize.  out_h is no multiple
    of the 16-row band; out_w = 23 and 1 take the byte stores, out_w = 64 at an odd address too, at an aligned one the 32-bit stores."""
    x, _ = _case(53, 37, 64, 6, "random")
    assert pp.resize_geometry(53, 37, 64)[:2] == (91, 64)
    top, left = 3, 64 - out_w
    kh, bh = pp.resample_axis(37, 64, left, out_w)
    kv, bv = pp.resample_axis(53, 91, top, out_h)
    mid = pp.resample_pass(x, *pp.resample_axis(37, 64), axis=-1)
    want = pp.resample_pass(mid, *pp.resample_axis(53, 91), axis=-2)[:, top:top + out_h, left:left + out_w]
    got, fenced = _launch(lib, x, out_h, out_w, kh, bh, kv, bv, offset=offset)
    assert fenced and int((got != want).sum()) == 0


# ---- 2. a plane's bytes do not depend on its batch-mates or on its place in the batch ----------------------------------------------
def test_rows_do_not_depend_on_their_neighbours(lib):
    h, w, n = 37, 53, 48
    x, want = _case(h, w, n, 3 * MAX_BATCH, "random")
    t = _tables(h, w, n)
    alone, _ = _launch(lib, x[9:12], n, n, *t)                                     # image 3 on its own
    order = np.arange(MAX_BATCH)[::-1].copy()
    shuffled, _ = _launch(lib, x.reshape(MAX_BATCH, 3, h, w)[order].reshape(-1, h, w), n, n, *t)
    assert np.array_equal(alone, want[9:12])
    assert np.array_equal(shuffled.reshape(MAX_BATCH, 3, n, n)[list(order).index(3)], alone)


# ---- 3. / 4. the engine -----------------------------------------------------------------------------------------------------------
MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


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


def _batch(h, w, B=MAX_BATCH, seed=0):
    g = torch.Generator().manual_seed(seed + h * 100 + w)
    x = torch.randint(0, 256, (B, 3, h, w), generator=g, dtype=torch.uint8)
    return x.cuda(), pp.resize_center_crop_u8(x, 48).cuda(), torch.randint(0, 10, (B,), generator=g).cuda()


@pytest.mark.parametrize("h,w", [(32, 32), (37, 53)])
def test_engine_calls_on_native_batches_equal_the_calls_on_the_resized_batch(engines, h, w):
    on, off = engines
    native, resized, labels = _batch(h, w)
    assert torch.equal(on.resize_u8(native), resized)
    assert torch.equal(on.predict(native), off.predict(resized))
    assert torch.equal(on.encode_image(native), off.encode_image(resized))
    assert torch.equal(on.visual_forward(native, save=False), off.visual_forward(resized, save=False))
    text = torch.nn.functional.normalize(torch.randn((7, on.arch.embed_dim), generator=torch.Generator().manual_seed(5)), dim=1).cuda()
    for a, b in zip(on.zeroshot(native, text, return_logits=True), off.zeroshot(resized, text, return_logits=True)):
        assert torch.equal(a, b)
    (l0, s0), (l1, s1) = on.forward_backward(native, labels), off.forward_backward(resized, labels)
    torch.cuda.synchronize()
    assert torch.equal(l0, l1) and torch.equal(s0, s1)
    assert torch.equal(on.grads, off.grads) and float(on.grads.abs().max()) > 0
    assert torch.equal(on.predict(native[:3].contiguous()), off.predict(resized[:3].contiguous()))      # a shorter batch, the tables cached


def test_probe_cache_fill_from_a_native_set(engines, tmp_path):
    from conftest import load_tiny_sd
    from test_mirror_api import tiny_config
    from pevit_amd.evaluation import _harness as h, full_model_finetune as fm
    from pevit_amd.evaluation.dataloader import TensorLoader, _Tensors
    ckpt = tmp_path / "tiny.pt"
    torch.save(load_tiny_sd(), ckpt)
    cfg = tiny_config(ckpt, classes=5)
    cfg.TRAIN.FREEZE_IMAGE_BACKBONE = True
    cfg.TEST.BATCH_SIZE_PER_GPU = cfg.TRAIN.BATCH_SIZE_PER_GPU = MAX_BATCH
    h._BACKBONES.clear()
    clf = fm.Classifier(cfg, 0).cuda(0)
    native, resized, labels = _batch(37, 53, B=12, seed=2)
    feats = []
    for images in (native, resized):
        fm.clear_feature_cache()
        cache = clf.cached(TensorLoader(_Tensors(images, labels), batch_size=MAX_BATCH, shuffle=False))
        assert cache is not None and cache.encoded == 12
        feats.append(cache.feats.clone())
    fm.clear_feature_cache(); h._BACKBONES.clear()
    assert torch.equal(feats[0], feats[1]) and float(feats[0].abs().max()) > 0


def test_refusals(engines):
    from pevit_amd._lib import PevitError
    on, off = engines
    native, resized, labels = _batch(32, 32)
    with pytest.raises(PevitError, match="images must be"):                       # resize off: the native batch is refused as before
        off.predict(native)
    with pytest.raises(PevitError, match="images must be"):
        off.forward_backward(native, labels)
    with pytest.raises(PevitError, match="images must be"):                       # resize on: f32 of another size is still refused
        on.predict(native.float())
    with pytest.raises(PevitError, match="8x"):                                    # beyond the kernel's range: refused before any launch
        on.predict(torch.zeros((2, 3, 400, 400), dtype=torch.uint8, device="cuda"))
    with pytest.raises(PevitError, match="capture_train_step"):
        on._steps, keep = 1, on._steps
        try:
            on.capture_train_step(native, labels, lr=0.01)
        finally:
            on._steps = keep
    from pevit_amd.engine import HipEngine
    bare = HipEngine(on.arch, "none", 10, MAX_BATCH)
    bare.set_input_resize(True)
    with pytest.raises(PevitError, match="set_input_normalization"):               # uint8 before the constants are known
        bare.predict(native)
    with pytest.raises(PevitError, match="ensure_batch"):
        on.resize_u8(torch.zeros((MAX_BATCH + 1, 3, 32, 32), dtype=torch.uint8, device="cuda"))


# ---- 5. the harness: engine resize against DATASET.RESIZE_ON_HOST ----------------------------------------------------------------------
def _harness_run(ckpt, host, resident, monkeypatch):
    from test_mirror_api import tiny_config
    from pevit_amd.evaluation import _harness as h, kadaptation_clip as kc
    from pevit_amd.evaluation import model as mirror
    from pevit_amd.evaluation.dataloader import TensorLoader, construct_dataloader
    cfg = tiny_config(ckpt, classes=5)
    cfg.DATASET.DATASET, cfg.DATASET.SYNTHETIC_SIZES, cfg.DATASET.LOADER_BATCH_SIZE = "synthetic", (40, 10), 8
    cfg.DATASET.SYNTHETIC_UINT8, cfg.DATASET.SYNTHETIC_SOURCE_SIZE = True, [32, 40]
    cfg.DATASET.RESIZE_ON_HOST, cfg.DATASET.RESIDENT = host, resident
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
        spec = tr.sample_spec()
        best, info = kc.train_task(tr, va, cfg)
    h._BACKBONES.clear(); mirror._ENGINES.clear()
    return best, batches, scored, spec


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "host-fed"])
def test_harness_engine_resize_equals_host_resize(gpu_required, resident, tmp_path, monkeypatch):
    from conftest import load_tiny_sd
    ckpt = tmp_path / "tiny.pt"
    torch.save(load_tiny_sd(), ckpt)
    b0, batches0, scored0, spec0 = _harness_run(ckpt, True, resident, monkeypatch)
    b1, batches1, scored1, spec1 = _harness_run(ckpt, False, resident, monkeypatch)
    assert spec0[0] == ((3, 48, 48), torch.uint8) and spec1[0] == ((3, 32, 40), torch.uint8)      # the native set stays native
    assert spec0[2].type == spec1[2].type == ("cuda" if resident else "cpu")
    assert batches0 == batches1 and len(batches0) == 2 * 4                  # 2 epochs x 30 train rows in batches of 8
    assert len(scored0) == len(scored1) == 4 and all(torch.equal(a, b) for a, b in zip(scored0, scored1))
    assert b0 == b1


# ---- the command line on a native-size set ----------------------------------------------------------------------------------------
def test_command_line_run_on_a_native_size_set_does_no_host_resize(gpu_required, tmp_path, monkeypatch):
    from conftest import load_tiny_sd
    from pevit_amd import preprocess
    from pevit_amd.commands import _finetune, kronecker_adaptation_clip as cmd
    from pevit_amd.config import default_config
    from pevit_amd.evaluation import _harness as h, model as mirror

    def no_host_resize(*a, **k):
        raise AssertionError("the run resized on the host")
    ckpt = tmp_path / "tiny.pt"
    torch.save(load_tiny_sd(), ckpt)
    model = tmp_path / "model.yaml"
    model.write_text(f"MODEL:\n  NAME: '{ckpt}'\n  SPEC:\n    EMBED_DIM: 64\nTRAIN:\n  END_EPOCH: 1\n  EXTRA_FINAL_TRAIN_EPOCH: 1\n"
                     "  NESTEROV: false\n  WD: 0.\nTEST:\n  METRIC: 'accuracy'\n")
    monkeypatch.setattr(_finetune, "config", default_config())
    monkeypatch.setattr(preprocess, "resize_center_crop_u8", no_host_resize)
    mirror._ENGINES.clear(); h._BACKBONES.clear()
    acc, info = cmd.main(["--model", str(model), "--no-tuning", "True", "--lr", "0.01", "--l2", "1e-6", "DATASET.DATASET", "synthetic",
                          "DATASET.NUM_CLASSES", "5", "OUTPUT_DIR", str(tmp_path / "out"), "TRAIN.IMAGE_SIZE", "[48, 48]",
                          "DATASET.SYNTHETIC_SIZES", "(40, 10)", "DATASET.SYNTHETIC_UINT8", "True", "DATASET.SYNTHETIC_SOURCE_SIZE", "[32, 32]"])
    h._BACKBONES.clear(); mirror._ENGINES.clear()
    assert 0.0 <= acc <= 100.0 and info["best_logits"].shape == (10, 5)
