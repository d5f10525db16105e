"""The zero-shot path on the GPU: the cosine head kernel (csrc/zeroshot.hip) against torch f64 on the same operands, its batch
invariance bit for bit, ``HipEngine.zeroshot`` / ``encode_image`` against ``predict`` on the tiny checkpoint, and the command.

Gate of the kernel: ``max_rel`` (conftest) of logits and of probabilities <= 1e-5, the project's gate for pure-f32 kernels; torch's
own f32 evaluation of exactly these inputs measures at most 6.2e-7 (logits) and 2.7e-6 (probabilities) against f64, so the
reference itself stays 4x inside it.
"""
import ctypes as C
import functools
import json
import logging
import re

import pytest
import torch

from conftest import load_tiny_sd, max_rel

pytestmark = pytest.mark.gpu

GATE = 1e-5
SCALE = 100.0


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pevit_amd import _lib
    return _lib.load()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(lib, rc):
    assert rc == 0, lib.pevit_last_error().decode()


def nan_buf(B, Cc):
    return torch.full((B, Cc), float("nan"), dtype=torch.float32, device="cuda")


def head(lib, feat, text, want_probs=True, want_logits=True):
    """pevit_op_zeroshot_head into NaN-filled buffers: an element the kernel does not write shows"""
    B, D = feat.shape
    Cc = text.shape[0]
    probs = nan_buf(B, Cc) if want_probs else None
    logits = nan_buf(B, Cc) if want_logits else None
    ok(lib, lib.pevit_op_zeroshot_head(S(), P(feat), P(text), SCALE, P(probs), P(logits), B, D, Cc))
    torch.cuda.synchronize()
    return probs, logits


# ---- 1. kernel parity ------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 64, 1),           # one class: probability exactly 1
          (3, 64, 5),           # partial row and class tiles
          (32, 512, 32),        # exact tiles
          (33, 512, 100),       # one row and four classes past a tile
          (37, 768, 211),       # B / 16 and ViT-L width with country211's class count
          (130, 512, 1000),     # many class tiles per wave
          (2, 1024, 1024)]      # both limits


@functools.lru_cache(maxsize=None)
def operands(B, D, Cc, hot):
    """(feat (B, D) f32, text (C, D) f32 unit rows, f64 logits, f64 probabilities), all on the CPU.  Features are randn * 3 with the
    last row zero; ``hot`` replaces one text row by the normalised feature row 0 (taken before the last row is zeroed): logit 100,
    a probability of nearly 1 against about e^-100."""
    g = torch.Generator().manual_seed(1000 * B + D + Cc)
    feat = torch.randn((B, D), generator=g) * 3
    text = torch.nn.functional.normalize(torch.randn((Cc, D), generator=g).double(), dim=1).float()
    if hot:
        text[Cc // 2] = torch.nn.functional.normalize(feat[0].double(), dim=0).float()
    feat[B - 1] = 0
    f = feat.double()
    logits = SCALE * (f / f.norm(dim=1, keepdim=True).clamp_min(1e-12)) @ text.double().t()
    return feat, text, logits, logits.softmax(dim=-1)


@pytest.mark.parametrize("hot", [False, True], ids=["plain", "hot"])
@pytest.mark.parametrize("B,D,Cc", SHAPES)
def test_head_matches_f64(lib, B, D, Cc, hot):
    feat, text, want_logits, want_probs = operands(B, D, Cc, hot)
    f, t = feat.cuda(), text.cuda()
    probs, logits = head(lib, f, t)
    e_l, e_p = max_rel(logits.cpu(), want_logits), max_rel(probs.cpu(), want_probs)
    sums = probs.double().sum(dim=1)
    print(f"({B}, {D}, {Cc}) {'hot' if hot else 'plain'}: max_rel logits {e_l:.3e} probs {e_p:.3e} (gate {GATE}), "
          f"|row sum - 1| {float((sums - 1).abs().max()):.3e}")
    assert torch.isfinite(probs).all() and torch.isfinite(logits).all()
    assert e_l <= GATE and e_p <= GATE
    assert float((sums - 1).abs().max()) <= 1e-6
    assert max_rel(probs[B - 1].cpu(), torch.full((Cc,), 1.0 / Cc, dtype=torch.float64)) <= GATE       # the zero row: uniform
    if Cc == 1:
        assert torch.equal(probs, torch.ones_like(probs))
    if hot and B > 1:
        assert float(probs[0, Cc // 2]) > 1 - 1e-6 and abs(float(logits[0, Cc // 2]) - 100.0) <= 100.0 * GATE
    # one output at a time: the same bits
    only_p, none_l = head(lib, f, t, want_logits=False)
    none_p, only_l = head(lib, f, t, want_probs=False)
    assert none_l is None and none_p is None
    assert torch.equal(only_p, probs) and torch.equal(only_l, logits)


# ---- 2. batch invariance ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,D,Cc", [(37, 512, 100), (130, 512, 1000)])
def test_a_row_alone_gives_the_bits_of_the_row_in_the_batch(lib, B, D, Cc):
    feat, text, _, _ = operands(B, D, Cc, False)
    f, t = feat.cuda(), text.cuda()
    probs, logits = head(lib, f, t)
    for row in (0, 15, 16, B - 1):
        p1, l1 = head(lib, f[row:row + 1].clone(), t)
        assert torch.equal(p1[0], probs[row]) and torch.equal(l1[0], logits[row]), row


# ---- 3. end to end on the tiny checkpoint ----------------------------------------------------------------------------------------
MAX_BATCH = 6


def tiny_engine(method, weight_format="bf16", max_batch=MAX_BATCH):
    """tiny_sd.npz (width 128, 2 layers, 48 px, D = 64) with random NON-ZERO adapters, a random head and running statistics"""
    from pevit_amd.engine import HipEngine, adapter_param_spec
    from pevit_amd.synth import ARCHS, randomize_adapters
    arch = ARCHS["tiny-128"]
    sd = {k: v for k, v in load_tiny_sd().items() if k.startswith("visual.")}
    ad = [(n, torch.zeros(s)) for n, s, _ in adapter_param_spec(method, arch.width, arch.layers)]
    randomize_adapters(ad, seed=3)
    sd.update(dict(ad))
    eng = HipEngine(arch, method, 10, max_batch, weight_format=weight_format)
    eng.load_state_dict(sd)
    g = torch.Generator().manual_seed(5)
    D = arch.embed_dim
    v = eng.param_views()
    with torch.no_grad():
        v["layers.0.weight"].copy_(((torch.rand((10, D), generator=g) * 2 - 1) / D ** 0.5).cuda())
        eng.running_mean.copy_((torch.randn(D, generator=g) * 0.3).cuda())
        eng.running_var.copy_((0.5 + torch.rand(D, generator=g)).cuda())
    return arch, eng


def tiny_images(arch, B, seed=3):
    from pevit_amd.synth import synth_batch
    return synth_batch(B, arch.resolution, 10, seed_img=seed, seed_lbl=seed + 1)[0].cuda()


def tiny_text(D, Cc=7, seed=9):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn((Cc, D), generator=g).double(), dim=1).float().cuda()


def check_zeroshot_against_predict(lib, eng, img, text):
    _, want_feat = eng.predict(img, return_features=True)
    probs, logits, feat = eng.zeroshot(img, text, return_logits=True, return_features=True)
    enc = eng.encode_image(img)
    probs_ws = eng.zeroshot(img, text)                      # features kept in the workspace slot
    torch.cuda.synchronize()
    assert torch.isfinite(want_feat).all() and float(want_feat.abs().max()) > 0
    assert torch.equal(feat, want_feat) and torch.equal(enc, want_feat)
    want_probs, want_logits = head(lib, want_feat, text)
    assert torch.equal(probs, want_probs) and torch.equal(logits, want_logits) and torch.equal(probs_ws, want_probs)
    out = torch.zeros_like(probs)
    assert eng.zeroshot(img, text, probs_out=out) is out
    torch.cuda.synchronize()
    assert torch.equal(out, want_probs)


@pytest.mark.parametrize("B", [1, 5, MAX_BATCH])
@pytest.mark.parametrize("method", ["none", "kadaptation"])
def test_zeroshot_and_encode_image_equal_predict_features_and_the_head(lib, method, B):
    arch, eng = tiny_engine(method)
    check_zeroshot_against_predict(lib, eng, tiny_images(arch, B), tiny_text(arch.embed_dim))


@pytest.mark.parametrize("weight_format", ["fp8", "f32-verify"])
def test_zeroshot_in_the_other_weight_formats(lib, weight_format):
    arch, eng = tiny_engine("kadaptation", weight_format=weight_format)
    check_zeroshot_against_predict(lib, eng, tiny_images(arch, 5), tiny_text(arch.embed_dim))


def test_zeroshot_from_uint8_pixels(lib):
    from pevit_amd import _lib
    arch, eng = tiny_engine("none", max_batch=4)
    text = tiny_text(arch.embed_dim)
    mean, std = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
    g = torch.Generator().manual_seed(11)
    u8 = torch.randint(0, 256, (4, 3, arch.resolution, arch.resolution), generator=g, dtype=torch.uint8).cuda()
    with pytest.raises(_lib.PevitError):
        eng.zeroshot(u8, text)                              # no preprocessing constants yet
    with pytest.raises(_lib.PevitError):
        eng.encode_image(u8)
    eng.set_input_normalization(mean, std)
    m = torch.tensor(mean, device="cuda").view(1, 3, 1, 1); s = torch.tensor(std, device="cuda").view(1, 3, 1, 1)
    f32 = ((u8.float() / 255 - m) / s).contiguous()
    a, fa = eng.zeroshot(u8, text, return_features=True)
    b, fb = eng.zeroshot(f32, text, return_features=True)
    ea, eb = eng.encode_image(u8), eng.encode_image(f32)
    torch.cuda.synchronize()
    assert float(a.abs().max()) > 0 and torch.equal(a, b) and torch.equal(fa, fb) and torch.equal(ea, eb) and torch.equal(ea, fa)


@pytest.mark.parametrize("method", ["none", "kadaptation"])
def test_zeroshot_moves_nothing_but_its_outputs(lib, method):
    from pevit_amd import _lib
    from pevit_amd.synth import synth_batch
    arch, eng = tiny_engine(method)
    text = tiny_text(arch.embed_dim)
    images, labels = synth_batch(MAX_BATCH, arch.resolution, 10, seed_img=3, seed_lbl=4)
    images, labels = images.cuda(), labels.cuda()
    eng.train_step(images, labels, lr=0.05, momentum=0.9, weight_decay=1e-3)      # non-zero gradients and momentum
    state = lambda: [t.clone() for t in (eng.params, eng.grads, eng.momentum, eng.running_mean, eng.running_var)]
    before = state()
    assert float(eng.grads.abs().max()) > 0
    first = eng.zeroshot(images[:3], text)
    eng.encode_image(images[:3])
    again = eng.zeroshot(images[:3], text)
    torch.cuda.synchronize()
    assert torch.equal(first, again)
    for a, b in zip(before, state()):
        assert torch.equal(a, b)
    # like every forward of the inference walk, neither leaves a saved forward behind
    for call in (lambda: eng.zeroshot(images, text), lambda: eng.encode_image(images)):
        eng.visual_forward(images, save=True)
        call()
        with pytest.raises(_lib.PevitError):
            eng.visual_backward(torch.ones((MAX_BATCH, arch.embed_dim), device="cuda"))
    # and refuses what the head cannot take, before the tower runs
    with pytest.raises(_lib.PevitError):
        eng.zeroshot(images, torch.zeros((1025, arch.embed_dim), device="cuda"))
    with pytest.raises(_lib.PevitError):
        eng.zeroshot(images, text[:, :32].contiguous())


# ---- 4. the command --------------------------------------------------------------------------------------------------------------
def test_command_on_the_tiny_checkpoint(lib, tmp_path, monkeypatch, caplog):
    import numpy as np
    from pevit_amd.commands import zeroshot as cmd
    from pevit_amd.config import default_config
    from pevit_amd.evaluation import clip_load, clip_zeroshot_evaluator, extract_features, extract_text_features
    sd = load_tiny_sd()
    ckpt = tmp_path / "tiny.pt"
    torch.save(sd, ckpt)
    model_yaml = tmp_path / "model.yaml"
    model_yaml.write_text(f"MODEL:\n  NAME: '{ckpt}'\n  SPEC:\n    EMBED_DIM: 64\nTEST:\n  METRIC: 'accuracy'\n")
    context, vocab = sd["positional_embedding"].shape[0], sd["token_embedding.weight"].shape[0]
    g = torch.Generator().manual_seed(21)
    class_names = [torch.randint(1, vocab, (3, context), generator=g) for _ in range(5)]      # 5 classes x 3 tokenised prompts
    monkeypatch.setattr(cmd, "config", default_config())
    argv = ["--model", str(model_yaml), "DATASET.DATASET", "synthetic", "DATASET.NUM_CLASSES", "5", "DATASET.ROOT", str(tmp_path),
            "OUTPUT_DIR", str(tmp_path / "out"), "TRAIN.IMAGE_SIZE", "[48, 48]", "DATASET.SYNTHETIC_SIZES", "(8, 11)"]
    with caplog.at_level(logging.INFO):
        result, probs, metric = cmd.main(argv, class_names=class_names)
    n_test = 11
    exp = "zeroshot_eval_wiki_False_wnh_False_wnd_False_gpt3_Falseagg_WIKI_AND_GPT3_gpt3count_1"
    j = json.load(open(tmp_path / "out" / "predictions" / exp / "synthetic.json"))
    p = np.asarray(j["predictions"][0])
    assert p.shape == (n_test, 5) and np.abs(p.sum(axis=1) - 1).max() <= 5e-6          # (five values rounded to six digits)
    assert j["n_shot"] == 0 and j["num_trainable_params"] == 0 and j["model_name"] == f"CLIP-{ckpt}"
    logged = [m for m in caplog.messages if m.startswith("=> TEST: ")]
    assert len(logged) == 1
    value = float(re.match(r"=> TEST: accuracy ([0-9.]+)% ", logged[0]).group(1))
    assert abs(value - 100 * result) <= 5e-4                                           # (printed with three digits)
    # the two-step route of the reference on the same model: extract_features + extract_text_features + the host evaluator
    cfg = cmd.config
    model, _ = clip_load.plain_load(str(ckpt), jit=False)
    feats, labels = extract_features(cfg, model, test_split_only=True)
    text_features = extract_text_features(cfg, None, model=model, class_names=class_names)
    want, want_probs, name = clip_zeroshot_evaluator(feats, text_features, labels, cfg)
    err = max_rel(probs, want_probs)
    print(f"command vs extract_features + host evaluator: max_rel {err:.3e} (gate {GATE}), accuracy {result} / {want}")
    assert name == metric == "accuracy" and feats.shape == (n_test, 64) and err <= GATE
    # the metric agrees unless an arg-max sits on a tie closer than the gate
    top2 = want_probs.double().topk(2, dim=1).values
    if float((top2[:, 0] - top2[:, 1]).min()) > 2 * GATE:
        assert result == want
