"""CPU-side checks of the text tower's boundary: pevit_text_create's limits and sizes, the refusals between text and image contexts
(host-side, before any launch), the new fixtures against the mirror's torch ``encode_text``, the per-class reduction over a stacked
tensor, ``text_engine_ok`` and the unchanged torch route of ``extract_text_features``, and the compiler-behaviour guard of the
causal attention kernel (tests/test_isa_hygiene.py's scan on attn_causal.hip)."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_tiny_sd
from test_isa_hygiene import CSRC, HIPCC, _kernels, _scan

from pevit_amd import _lib
from pevit_amd.config import default_config
from pevit_amd.evaluation.feature import extract_text_features, reduce_class_features
from pevit_amd.evaluation.model import build_model
from pevit_amd.synth import VitArch, synth_state_dict
from pevit_amd.text_engine import text_engine_ok

TEXT_TAGS = ["w128_l2_n77", "w256_l3_n77", "w128_l2_n8", "w512_l12_n77"]
BF16, FP8, F32V, FP8ACT = 0, 1, 2, 3


def load_text_fixture(tag):
    """(meta, tensors, state-dict) of a fixture of tests/golden/make_golden_text.py; the weights are rebuilt from (arch, seed)"""
    with open(os.path.join(GOLDEN, f"text_{tag}.json")) as f:
        meta = json.load(f)
    z = np.load(os.path.join(GOLDEN, f"text_{tag}.npz"))
    t = {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}
    arch = VitArch(*meta["arch"])
    sd = synth_state_dict(arch, seed=meta["seed"], text_tower=True)
    sd = {k: (v.half().float() if v.dim() > 0 else v) for k, v in sd.items()}
    return meta, t, arch, sd


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def text_ctx(lib, *dims):
    ctx = C.c_void_p()
    d = _lib.PevitTextDims(*dims)
    return lib.pevit_text_create(C.byref(d), C.byref(ctx)), ctx


@pytest.mark.parametrize("dims", [(64, 12, 77, 49408, 512, BF16), (1152, 12, 77, 49408, 512, BF16), (512, 12, 0, 49408, 512, BF16),
                                  (512, 12, 129, 49408, 512, BF16), (512, 12, 77, 49408, 12, BF16), (512, 12, 77, 49408, 512, FP8),
                                  (512, 12, 77, 49408, 512, FP8ACT)])
def test_text_create_refuses_with_a_message(lib, dims):
    rc, _ = text_ctx(lib, *dims)
    assert rc != 0
    assert len(lib.pevit_last_error()) > 0 and b"text_create" in lib.pevit_last_error()


def test_text_create_sizes(lib):
    rc, ctx = text_ctx(lib, 512, 12, 77, 49408, 512, BF16)
    assert rc == 0, lib.pevit_last_error()
    assert lib.pevit_arena_bytes(ctx) > 49408 * 512 * 4               # the f32 table alone
    w8, w256 = lib.pevit_workspace_bytes(ctx, 8), lib.pevit_workspace_bytes(ctx, 256)
    assert 0 < w8 < w256
    # inference layout: smaller than the training layout of an image context of the same width / depth / row count: 82 prompts of
    # 77 tokens against 77 images of 9 x 9 + 1 = 82 tokens
    d = _lib.PevitDims(512, 12, 32, 288, 512, _lib.METHOD_IDS["none"], 4, 10, BF16)          # grid 9 x 9 + 1 = 82 tokens
    img = C.c_void_p()
    assert lib.pevit_ctx_create(C.byref(d), C.byref(img)) == 0, lib.pevit_last_error()
    assert lib.pevit_workspace_bytes(ctx, 82) < lib.pevit_workspace_bytes(img, 77)            # 82 * 77 rows each
    rcv, ctxv = text_ctx(lib, 512, 12, 77, 49408, 512, F32V)
    assert rcv == 0 and lib.pevit_workspace_bytes(ctxv, 256) > w256          # f32 activations
    for c in (ctx, img, ctxv):
        lib.pevit_ctx_destroy(c)


def test_image_entry_points_refuse_a_text_context_and_encode_text_an_image_context(lib):
    rc, ctx = text_ctx(lib, 128, 2, 77, 512, 64, BF16)
    assert rc == 0
    N = None
    calls = {
        "pevit_visual_forward": (ctx, N, N, N, 1, 0), "pevit_visual_forward_u8": (ctx, N, N, N, 1, 0),
        "pevit_predict": (ctx, N, N, N, N, N, N, 1), "pevit_predict_u8": (ctx, N, N, N, N, N, N, 1),
        "pevit_train_forward_backward": (ctx, N, N, N, N, N, 1, N, N, 2),
        "pevit_train_forward_backward_u8": (ctx, N, N, N, N, N, 1, N, N, 2),
        "pevit_train_forward_backward_bce": (ctx, N, N, N, N, N, 1, N, N, 2),
        "pevit_train_forward_backward_bce_u8": (ctx, N, N, N, N, N, 1, N, N, 2),
        "pevit_head_forward_backward": (ctx, N, N, N, N, N, 1, N, N, N, 2),
        "pevit_head_forward_backward_bce": (ctx, N, N, N, N, N, 1, N, N, N, 2),
        "pevit_visual_backward": (ctx, N, N, 1), "pevit_visual_backward_part": (ctx, N, N, 1, 2, 0),
        "pevit_transformer_backward": (ctx, N, N, N, 1), "pevit_blocks_backward": (ctx, N, N, N, 1, 0, 2),
        "pevit_attention_backward": (ctx, N, 0, N, N, 1),
        "pevit_transformer_forward": (ctx, N, N, N, 1, 0), "pevit_blocks_forward": (ctx, N, N, N, 1, 0, 0, 2),
        "pevit_attention_forward": (ctx, N, 0, N, N, 1, 0, N, 0),
        "pevit_load_stem": (ctx, N, N, N, N, N, N, N, N, N),
    }
    for name, args in calls.items():
        assert getattr(lib, name)(*args) != 0, name
        assert b"text context" in lib.pevit_last_error(), (name, lib.pevit_last_error())
    lib.pevit_ctx_destroy(ctx)
    d = _lib.PevitDims(128, 2, 16, 48, 64, _lib.METHOD_IDS["none"], 4, 10, BF16)
    img = C.c_void_p()
    assert lib.pevit_ctx_create(C.byref(d), C.byref(img)) == 0
    assert lib.pevit_encode_text(img, None, None, None, 1) != 0
    assert b"image context" in lib.pevit_last_error()
    assert lib.pevit_load_text_stem(img, None, None, None, None, None, None) != 0
    assert b"not a text context" in lib.pevit_last_error()
    lib.pevit_ctx_destroy(img)
    # an unbound text context refuses to run
    rc, ctx = text_ctx(lib, 128, 2, 77, 512, 64, BF16)
    assert lib.pevit_encode_text(ctx, None, None, None, 1) != 0 and b"not bound" in lib.pevit_last_error()
    lib.pevit_ctx_destroy(ctx)


@pytest.mark.parametrize("tag", TEXT_TAGS)
def test_mirror_encode_text_reproduces_the_fixture(tag):
    meta, t, arch, sd = load_text_fixture(tag)
    assert meta["arch"][6:] == [arch.text_width, arch.text_layers, arch.context_length, arch.vocab_size]
    tokens = t["tokens"]
    N = arch.context_length
    # the token edge cases every fixture carries: the end-of-text maximum at the last position, at position 0, on both sides of a
    # 16-row tile boundary where the context has one, and a prompt whose maximum occurs twice (argmax takes the first)
    eot = tokens.argmax(dim=-1).tolist()
    assert eot[0] == N - 1 and eot[1] == 0
    if N > 17:
        assert eot[2] == 15 and eot[3] == 16
    last = tokens[-1]
    assert int((last == last.max()).sum()) == 2 and eot[-1] == int((last == last.max()).nonzero()[0])
    model = build_model(dict(sd))
    with torch.no_grad():
        feats = model.encode_text(tokens)
    assert torch.allclose(feats, t["text_features"], atol=1e-6, rtol=1e-6)
    for leg in ("weights", "operands"):
        assert 0.0 < meta["floor"][leg]["max_rel"] < 2e-2 and 0.0 < meta["floor"][leg]["rel_err"] < 2e-2


def _loop_reduce(feats, sizes):
    cols, o = [], 0
    for n in sizes:
        e = feats[o:o + n]; o += n
        e = e / e.norm(dim=-1, keepdim=True)
        m = e.mean(dim=0)
        cols.append(m / m.norm())
    return torch.stack(cols, dim=1)


@pytest.mark.parametrize("tag", TEXT_TAGS)
def test_stacked_reduction_equals_the_per_class_loop(tag):
    meta, t, _, _ = load_text_fixture(tag)
    sizes = meta["class_sizes"]
    if tag == "w512_l12_n77":
        assert {1, 3, 4} <= set(sizes)
    index = torch.cat([torch.full((n,), i, dtype=torch.int64) for i, n in enumerate(sizes)])
    got = reduce_class_features(t["text_features"], index, len(sizes))
    assert got.shape == (t["text_features"].shape[1], len(sizes))
    assert torch.allclose(got, _loop_reduce(t["text_features"], sizes), atol=1e-6, rtol=1e-6)
    assert torch.allclose(got, t["zeroshot_weights"], atol=1e-6, rtol=1e-6)
    # rows of a class need not be adjacent
    perm = torch.randperm(index.numel(), generator=torch.Generator().manual_seed(3))
    assert torch.allclose(reduce_class_features(t["text_features"][perm], index[perm], len(sizes)), got, atol=1e-6, rtol=1e-6)


def test_text_engine_ok_is_a_pure_predicate():
    tiny = build_model(load_tiny_sd())
    for p in tiny.parameters():
        p.requires_grad = False
    assert not text_engine_ok(tiny)                        # text width 64
    _, _, _, sd = load_text_fixture("w128_l2_n77")
    model = build_model(dict(sd))
    for p in model.parameters():
        p.requires_grad = False
    assert not text_engine_ok(model)                       # a CPU model
    with pytest.raises(_lib.PevitError):
        model.encode_text_engine(torch.zeros((1, 77), dtype=torch.int64))
    if torch.cuda.is_available():
        model = model.cuda()
        assert text_engine_ok(model)
        model.transformer.resblocks[1].mlp.c_fc.bias.requires_grad = True
        assert not text_engine_ok(model)                   # a trainable text parameter
    else:
        # the remaining conditions without a device: everything but "on a GPU" holds, and a trainable parameter is named first
        from pevit_amd.text_engine import text_engine_refusal
        assert "GPU" in text_engine_refusal(model)
        model.ln_final.weight.requires_grad = True
        assert not text_engine_ok(model)


def test_engine_key_changes_nothing_where_the_engine_cannot_run():
    """TEXT_TOWER_ENGINE on a model the engine refuses (text width 64, and on this machine possibly the CPU): today's result, exactly"""
    z = np.load(os.path.join(GOLDEN, "tiny_text.npz"))
    tokens = torch.from_numpy(z["tokens"])
    model = build_model(load_tiny_sd())
    for p in model.parameters():
        p.requires_grad = False
    cfg = default_config()
    assert cfg.TRAIN.TEXT_TOWER_ENGINE is False
    cfg.MODEL.SPEC.TEXT.CONTEXT_LENGTH = 8
    names = [tokens[c] for c in range(10)]
    before = extract_text_features(cfg, None, model=model, return_numpy=True, class_names=names)
    cfg.TRAIN.TEXT_TOWER_ENGINE = True
    after = extract_text_features(cfg, None, model=model, return_numpy=True, class_names=names)
    assert np.array_equal(before, after)
    np.testing.assert_allclose(after, z["zeroshot_weights"], atol=1e-6, rtol=1e-6)


def test_causal_kernel_has_no_drained_loads_and_no_wait_between_stores(tmp_path):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    s = tmp_path / "attn_causal.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "--cuda-device-only", "-S",
                    os.path.join(CSRC, "attn_causal.hip"), "-o", str(s)], check=True, capture_output=True, timeout=900)
    kernels = {n: ins for n, ins in _kernels(s.read_text()).items() if "attn_causal_fwd_kernel" in n}
    assert len(kernels) == 4                               # KT32 = 1 .. 4
    for name, ins in kernels.items():
        drained, waits, _ = _scan(ins)
        assert drained == 0, f"{name}: {drained} loads are drained with vmcnt(0) right behind their request"
        assert waits == 0, f"{name}: {waits} s_waitcnt vmcnt(0) between the first and the last store"
        assert not any(x.startswith("scratch_") for x in ins), f"{name}: scratch traffic"
