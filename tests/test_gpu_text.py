"""The CLIP text tower on the engine: the causal attention kernel one launch at a time (parity with torch's masked softmax attention,
the exact first row, no leak from later tokens, the refused token counts), ``TextEngine.encode`` against the fixtures recorded from
the reference (tests/golden/make_golden_text.py) in bf16 and in the f32 verification mode, chunking and repeatability, the host's
token-range check, and ``Classifier(INIT_HEAD_WITH_TEXT_ENCODER)`` through both routes of ``extract_text_features``.

Gates: attention output < 1.5e-2 of the largest magnitude (test_gpu_ops.py's gate for the unmasked kernel: bf16 probabilities and a
bf16 result); features < max(2e-2, FLOOR_C x the bf16 floor the reference recorded on itself) (conftest.floor_gate); f32 verification
mode < 2e-4 (12 layers: 2e-3), the F32_LOGITS / 10 x F32_LOGITS of test_gpu_verify.py."""
import ctypes as C

import pytest
import torch

from conftest import floor_gate, max_rel
from test_text_host import TEXT_TAGS, load_text_fixture

pytestmark = pytest.mark.gpu

ATTN_GATE = 1.5e-2
STATED_FEATURES = 2e-2
F32_LOGITS = 2e-4


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


def rnd(*shape, scale=1.0, seed=0, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def causal(lib, q, k, v, B, H, N):
    out = torch.zeros((B * N, H * 64), dtype=torch.bfloat16, device="cuda")
    rc = lib.pevit_op_attn_fwd_causal(S(), P(q), P(k), P(v), P(out), H * 64, B, H, N)
    assert rc == 0, lib.pevit_last_error().decode()
    torch.cuda.synchronize()
    return out


def rows(x, B, H, N):
    """(B*H, N, 64) head layout -> [B*N][H*64] rows"""
    return x.view(B, H, N, 64).permute(0, 2, 1, 3).reshape(B * N, H * 64)


def qkv(B, H, N, seed=0):
    return (rnd(B * H, N, 64, seed=seed + 1, scale=0.35, dtype=torch.bfloat16), rnd(B * H, N, 64, seed=seed + 2, dtype=torch.bfloat16),
            rnd(B * H, N, 64, seed=seed + 3, dtype=torch.bfloat16))


SHAPES = [(3, 2, 77), (2, 8, 77), (1, 12, 77), (2, 1, 1), (1, 2, 8), (2, 2, 16), (2, 2, 17), (1, 3, 33), (2, 2, 64), (1, 2, 65),
          (1, 1, 96), (1, 2, 128)]


@pytest.mark.parametrize("B,H,N", SHAPES)
def test_causal_attention_matches_masked_softmax(lib, B, H, N):
    q, k, v = qkv(B, H, N)
    out = causal(lib, q, k, v, B, H, N)
    mask = torch.full((N, N), float("-inf"), device="cuda").triu_(1)
    p = torch.softmax(q.float() @ k.float().transpose(1, 2) + mask, dim=-1)          # q already carries the 1/8
    ref = rows(p @ v.float(), B, H, N)
    err = max_rel(out.float().cpu(), ref.cpu())
    print(f"causal attention B={B} H={H} N={N}: max_rel {err:.3g}")
    assert err < ATTN_GATE


@pytest.mark.parametrize("B,H,N", SHAPES)
def test_first_row_is_v_row_0_bit_for_bit(lib, B, H, N):
    """one key: probability 1, whatever the tolerance"""
    q, k, v = qkv(B, H, N, seed=10)
    out = causal(lib, q, k, v, B, H, N)
    got = out.view(B, N, H, 64)[:, 0].reshape(B * H, 64)
    assert torch.equal(got.view(torch.int16), v[:, 0].contiguous().view(torch.int16))


@pytest.mark.parametrize("n0", [1, 16, 17, 40, 76])
def test_no_leak_from_the_future(lib, n0):
    """two calls that differ only in q, k, v rows >= n0 give bit-identical output rows < n0"""
    B, H, N = 2, 3, 77
    q, k, v = qkv(B, H, N, seed=20)
    q2, k2, v2 = (t.clone() for t in (q, k, v))
    for t, other in zip((q2, k2, v2), qkv(B, H, N, seed=30)):
        t[:, n0:] = 3.0 * other[:, n0:]
    a = causal(lib, q, k, v, B, H, N).view(B, N, H * 64)
    b = causal(lib, q2, k2, v2, B, H, N).view(B, N, H * 64)
    assert torch.equal(a[:, :n0].contiguous().view(torch.int16), b[:, :n0].contiguous().view(torch.int16))
    assert not torch.equal(a[:, n0:], b[:, n0:])                   # (the later rows did change)


@pytest.mark.parametrize("N", [0, 129])
def test_token_counts_outside_the_range_are_refused(lib, N):
    q, k, v = qkv(1, 1, 4)
    out = torch.full((4, 64), 7.0, dtype=torch.bfloat16, device="cuda")
    assert lib.pevit_op_attn_fwd_causal(S(), P(q), P(k), P(v), P(out), 64, 1, 1, N) != 0
    assert b"outside [1,128]" in lib.pevit_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                # nothing was launched


# ---------------------------------------------------------------------------------------------------------------- the tower
_ENGINES = {}


def engine(tag, weight_format="bf16", max_prompts=64):
    from pevit_amd.text_engine import TextEngine
    key = (tag, weight_format, max_prompts)
    if key not in _ENGINES:
        _, _, arch, sd = load_text_fixture(tag)
        eng = TextEngine(arch, max_prompts=max_prompts, device="cuda:0", weight_format=weight_format)
        eng.load_state_dict(sd)
        _ENGINES[key] = eng
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _release_engines():
    yield
    _ENGINES.clear()


def feature_gate(meta):
    return floor_gate(STATED_FEATURES, max(meta["floor"][leg]["max_rel"] for leg in ("weights", "operands")))


@pytest.mark.parametrize("tag", TEXT_TAGS)
def test_encode_matches_the_reference_features(lib, tag):
    meta, t, arch, _ = load_text_fixture(tag)
    feats = engine(tag).encode(t["tokens"])
    assert feats.shape == t["text_features"].shape and feats.dtype == torch.float32 and feats.is_cuda
    err, floor = max_rel(feats.cpu(), t["text_features"]), max(meta["floor"][leg]["max_rel"] for leg in ("weights", "operands"))
    print(f"text {tag}: engine max_rel {err:.3g}, reference bf16 floor {floor:.3g}, gate {feature_gate(meta):.3g}")
    assert err < feature_gate(meta)
    # device tokens and another integer dtype take the same path
    again = engine(tag).encode(t["tokens"].to(torch.int32).cuda())
    assert torch.equal(again, feats)


@pytest.mark.parametrize("tag", TEXT_TAGS)
def test_encode_f32_verification_mode(lib, tag):
    meta, t, arch, _ = load_text_fixture(tag)
    feats = engine(tag, "f32-verify").encode(t["tokens"])
    err = max_rel(feats.cpu(), t["text_features"])
    gate = F32_LOGITS if arch.text_layers < 12 else 10 * F32_LOGITS
    print(f"text {tag} f32-verify: max_rel {err:.3g}, gate {gate:.3g}")
    assert err < gate


def test_chunked_calls_and_repeatability(lib):
    tag = "w128_l2_n77"
    meta, t, arch, _ = load_text_fixture(tag)
    tokens = torch.cat([t["tokens"], t["tokens"][:2]])                   # 9 prompts: calls of 4, 4, 1
    ref = torch.cat([t["text_features"], t["text_features"][:2]])
    eng = engine(tag, max_prompts=4)
    a = eng.encode(tokens)
    err = max_rel(a.cpu(), ref)
    print(f"text {tag}, 9 prompts in chunks of 4: max_rel {err:.3g}")
    assert err < feature_gate(meta)
    assert torch.equal(eng.encode(tokens), a)                            # the same call twice: bit-identical
    assert eng.encode(tokens[:0]).shape == (0, arch.embed_dim)


def test_bad_tokens_are_refused_on_the_host(lib):
    from pevit_amd._lib import PevitError
    tag = "w128_l2_n8"
    _, t, arch, _ = load_text_fixture(tag)
    eng = engine(tag)
    for bad in (arch.vocab_size + 5, -1):
        for dev in ("cpu", "cuda"):
            tok = t["tokens"].clone()
            tok[1, 2] = bad
            with pytest.raises(PevitError, match="outside the vocabulary"):
                eng.encode(tok.to(dev))
    with pytest.raises(PevitError, match="expected"):
        eng.encode(t["tokens"][:, :-1])
    with pytest.raises(PevitError, match="integer"):
        eng.encode(t["tokens"].float())


def test_classifier_head_through_both_routes(lib, tmp_path):
    from pevit_amd.config import default_config
    from pevit_amd.evaluation import _harness
    from pevit_amd.evaluation.kadaptation_clip import Classifier
    from pevit_amd.optim import build_optimizer
    from pevit_amd.text_engine import TextEngine
    tag = "w128_l2_n77"
    meta, t, arch, sd = load_text_fixture(tag)
    path = tmp_path / "text128.pt"
    torch.save(sd, path)
    sizes, names, o = meta["class_sizes"], [], 0
    for n in sizes:
        names.append(t["tokens"][o:o + n]); o += n

    def build(engine_route):
        _harness._BACKBONES.clear(); _harness._ZEROSHOT.clear()
        cfg = default_config()
        cfg.MODEL.NAME = str(path)
        cfg.MODEL.SPEC.EMBED_DIM = arch.embed_dim
        cfg.MODEL.SPEC.TEXT.CONTEXT_LENGTH = arch.context_length
        cfg.DATASET.NUM_CLASSES = len(sizes)
        cfg.DATASET.CLASS_NAMES = names
        cfg.TRAIN.NESTEROV = False
        cfg.TRAIN.BATCH_SIZE_PER_GPU = 4
        cfg.TEST.BATCH_SIZE_PER_GPU = 4
        cfg.TRAIN.INIT_HEAD_WITH_TEXT_ENCODER = True
        cfg.TRAIN.TEXT_TOWER_ENGINE = engine_route
        return cfg, Classifier(cfg, 0).cuda(0)

    cfg, clf = build(False)
    with torch.no_grad():        # today's route, restated: one torch call per class
        cols = []
        for c in names:
            e = clf.backbone.encode_text(c.cuda())
            e = e / e.norm(dim=-1, keepdim=True)
            m = e.mean(dim=0)
            cols.append(m / m.norm())
        today = torch.stack(cols, dim=1).T.contiguous()
    assert torch.equal(clf.layers[0].weight.detach(), today)
    del clf
    cfg, clf = build(True)
    err = max_rel(clf.layers[0].weight.detach().cpu(), today.cpu())
    print(f"zero-shot head, engine route against the torch route: max_rel {err:.3g}, gate {feature_gate(meta):.3g}")
    assert 0.0 < err < feature_gate(meta)
    assert float(clf.layers[0].bias.abs().max()) == 0.0
    assert not any(isinstance(v, TextEngine) for v in vars(clf.backbone).values())      # released after the extraction
    # a fused train step afterwards (the backbone stays in eval mode, as in the reference's train_one)
    opt = build_optimizer(cfg, clf)
    crit = torch.nn.CrossEntropyLoss().cuda(0)
    assert clf.can_fuse(crit, opt)
    images = rnd(4, 3, arch.resolution, arch.resolution, seed=5)
    labels = torch.tensor([0, 1, 2, 1], device="cuda")
    logits, loss = clf.fused_train_step(images, labels, opt)
    torch.cuda.synchronize()
    assert logits.shape == (4, len(sizes)) and bool(torch.isfinite(logits).all()) and bool(torch.isfinite(loss).all())
    _harness._BACKBONES.clear(); _harness._ZEROSHOT.clear()
