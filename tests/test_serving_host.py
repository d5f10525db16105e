"""Inference-only contexts and adapter checkpoints, without a GPU: the two C entries, the sizes ``pevit_infer_create`` promises
(include/pevit_hip.h) against the training context of the same dims, and ``pevit_amd/adapter_io.py`` on CPU tensors.

The arena bound is what ``carve_block_arena`` / ``pevit_ctx_create`` of csrc/ctx.hip give the backward alone: per layer the
transposed copies wqkvT (E x NQ), woT (E x E), wfcT and wprT (4 E x E each), and projT (E x D) once.  The workspace bound is the
sum of the slots the inference walk touches, computed here from the dims (``workspace_bound``)."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

from pevit_amd import _lib, adapter_io
from pevit_amd.engine import adapter_param_spec
from pevit_amd.synth import ARCHS

METHODS = ["kadaptation", "lora", "adapter", "compacter", "none"]
FORMATS = ["bf16", "fp8", "fp8-act", "f32-verify"]
CLASSES = 10


def creatable(method, weight_format):
    return not (weight_format in ("fp8", "fp8-act") and method in ("adapter", "compacter"))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def dims_of(arch, method, weight_format, classes=CLASSES, layers=None):
    return _lib.PevitDims(arch.width, layers or arch.layers, arch.patch, arch.resolution, arch.embed_dim, _lib.METHOD_IDS[method], 4,
                          classes, _lib.WEIGHT_FORMATS[weight_format])


def create(lib, creator, dims):
    ctx = C.c_void_p()
    rc = getattr(lib, creator)(C.byref(dims), C.byref(ctx))
    return rc, ctx


def both(lib, arch, method, weight_format, **kw):
    d = dims_of(arch, method, weight_format, **kw)
    (rt, train), (ri, infer) = create(lib, "pevit_ctx_create", d), create(lib, "pevit_infer_create", d)
    assert rt == 0 and ri == 0, lib.pevit_last_error()
    return train, infer


# ---- the C entries --------------------------------------------------------------------------------------------------------------
def test_the_two_entries_are_exported_declared_and_typed(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pevit_hip.h")).read(), flags=re.S)
    for name, args in (("pevit_infer_create", 2), ("pevit_set_infer_params", 3)):
        assert hasattr(lib, name) and re.search(r"\bint\s+%s\s*\(" % name, header), name
        res, argtypes = _lib.SIGNATURES[name]
        assert res is C.c_int and len(argtypes) == args
    ctx = C.c_void_p()
    assert lib.pevit_infer_create(None, C.byref(ctx)) != 0 and b"null argument" in lib.pevit_last_error()
    assert lib.pevit_set_infer_params(None, None, 1) != 0
    # a training context takes pevit_set_params, not this; an inference-only one refuses pevit_set_params (nothing is read or launched)
    train, infer = both(lib, ARCHS["tiny-128"], "lora", "bf16")
    fake = C.c_void_p(256)
    assert lib.pevit_set_infer_params(train, fake, 3) != 0 and b"not an inference-only context" in lib.pevit_last_error()
    assert lib.pevit_set_params(infer, fake, fake, fake, fake) != 0 and b"inference-only context" in lib.pevit_last_error()
    for bad in (0, CLASSES + 1):
        assert lib.pevit_set_infer_params(infer, fake, bad) != 0 and b"num_classes" in lib.pevit_last_error()
    n_tower = lib.pevit_num_tower_params(infer)
    assert n_tower == lib.pevit_num_tower_params(train)
    for c in (CLASSES, 3):          # the head offsets follow the class count
        assert lib.pevit_set_infer_params(infer, fake, c) == 0
        assert lib.pevit_num_params(infer) == n_tower + c * ARCHS["tiny-128"].embed_dim + c
    for ctx in (train, infer):
        lib.pevit_ctx_destroy(ctx)


def test_infer_create_refuses_exactly_what_ctx_create_refuses(lib):
    bad = [_lib.PevitDims(100, 12, 32, 224, 512, 0, 4, 100), _lib.PevitDims(768, 12, 32, 225, 512, 0, 4, 100),
           _lib.PevitDims(768, 12, 32, 224, 512, 9, 4, 100), _lib.PevitDims(768, 12, 32, 224, 512, 1, 64, 100),
           _lib.PevitDims(768, 12, 8, 224, 512, 0, 4, 100), _lib.PevitDims(768, 0, 32, 224, 512, 0, 4, 100),
           _lib.PevitDims(768, 12, 32, 224, 510, 0, 4, 100), _lib.PevitDims(768, 12, 32, 224, 512, 0, 4, 0),
           _lib.PevitDims(768, 12, 32, 224, 512, 0, 4, 100, 7), _lib.PevitDims(1152, 12, 32, 224, 512, 0, 4, 100)]
    bad += [dims_of(ARCHS["tiny-128"], m, f) for m in ("adapter", "compacter") for f in ("fp8", "fp8-act")]
    for d in bad:
        rt, _ = create(lib, "pevit_ctx_create", d)
        want = lib.pevit_last_error().split(b": ", 1)[1]
        ri, _ = create(lib, "pevit_infer_create", d)
        assert rt != 0 and ri != 0
        assert lib.pevit_last_error() == b"infer_create: " + want
    for arch_name in ARCHS:
        for m in METHODS:
            for f in FORMATS:
                d = dims_of(ARCHS[arch_name], m, f)
                (rt, train), (ri, infer) = create(lib, "pevit_ctx_create", d), create(lib, "pevit_infer_create", d)
                assert (rt == 0) == (ri == 0) == creatable(m, f), (arch_name, m, f)
                if rt == 0:
                    lib.pevit_ctx_destroy(train); lib.pevit_ctx_destroy(infer)


# ---- the arena ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight_format", ["bf16", "f32-verify"])
def test_the_arena_drops_every_transposed_copy(lib, weight_format):
    es = 4 if weight_format == "f32-verify" else 2
    for arch_name, a in ARCHS.items():
        E, L, D = a.width, a.layers, a.embed_dim
        NQ = 3 * E + 64
        for m in METHODS:
            train, infer = both(lib, a, m, weight_format)
            t, i = lib.pevit_arena_bytes(train), lib.pevit_arena_bytes(infer)
            assert 0 < i <= t - L * (E * NQ + E * E + 8 * E * E) * es - E * D * es, (arch_name, m, t, i)
            lib.pevit_ctx_destroy(train); lib.pevit_ctx_destroy(infer)


@pytest.mark.parametrize("weight_format", ["fp8", "fp8-act"])
def test_the_fp8_arena_is_smaller(lib, weight_format):
    for arch_name, a in ARCHS.items():
        for m in ("kadaptation", "lora", "none"):
            train, infer = both(lib, a, m, weight_format)
            assert 0 < lib.pevit_arena_bytes(infer) < lib.pevit_arena_bytes(train), (arch_name, m)
            lib.pevit_ctx_destroy(train); lib.pevit_ctx_destroy(infer)


# ---- the workspace --------------------------------------------------------------------------------------------------------------
def workspace_bound(lib, ctx, a, method, weight_format, B, classes=CLASSES):
    src = open(os.path.join(ROOT, "pevit_amd", "csrc", "kernels.h")).read()
    slab_floats = eval(re.search(r"constexpr int PEVIT_SK_SLAB_FLOATS = ([0-9* ]+);", src).group(1))
    es = 4 if weight_format == "f32-verify" else 2
    slots = 0 if weight_format == "f32-verify" else lib.pevit_op_gemm_sk_slots()
    E, D, H = a.width, a.embed_dim, a.heads
    N, G2 = a.tokens, a.tokens - 1
    Kpatch = -(-3 * a.patch * a.patch // 64) * 64
    T = B * N
    total = lib.pevit_workspace_state_bytes(ctx) + slots * slab_floats * 4
    total += T * E * 4 * 5                        # x_in, its alternate, x_mid, x_final, xpre
    total += T * E * es * 10                      # xn1, q | k | v, attn_out, xn2, g (4)
    total += T * 64 * 4 + B * H * N * 4           # t, lse
    if method in ("adapter", "compacter"):
        total += T * E * (4 + es) + 2 * T * 64 * es + 2 * T * 4
    if weight_format == "fp8-act":
        total += 2 * T * E
    total += B * G2 * Kpatch * es + B * E * es + 2 * B * D * 4 + D * 4 + 2 * B * classes * 4
    return total + 64 * 256


@pytest.mark.parametrize("weight_format", FORMATS)
def test_the_workspace_is_below_the_training_one_and_below_its_bound(lib, weight_format):
    for arch_name in ("tiny-128", "tiny-256", "tiny-n257", "ViT-B/32", "ViT-L/14"):
        a = ARCHS[arch_name]
        for m in METHODS:
            if not creatable(m, weight_format):
                continue
            train, infer = both(lib, a, m, weight_format)
            for B in (1, 5, 128):
                t, i = lib.pevit_workspace_bytes(train, B), lib.pevit_workspace_bytes(infer, B)
                assert lib.pevit_workspace_state_bytes(infer) < i < t, (arch_name, m, B, t, i)
                assert i <= workspace_bound(lib, infer, a, m, weight_format, B), (arch_name, m, B, i)
            lib.pevit_ctx_destroy(train); lib.pevit_ctx_destroy(infer)


def test_the_workspace_does_not_depend_on_the_layer_count(lib):
    a = ARCHS["tiny-256"]
    for m in METHODS:
        for f in ("bf16", "f32-verify"):
            ctxs = [create(lib, "pevit_infer_create", dims_of(a, m, f, layers=L))[1] for L in (1, 3, 24)]
            for B in (1, 5, 128):
                assert len({lib.pevit_workspace_bytes(c, B) for c in ctxs}) == 1, (m, f, B)
            for c in ctxs:
                lib.pevit_ctx_destroy(c)


# ---- checkpoints on CPU tensors ---------------------------------------------------------------------------------------------------
def synthetic_ckpt(method="kadaptation", arch_name="tiny-128", classes=7, lora_rank=4, seed=0, **meta_over):
    a = ARCHS[arch_name]
    g = torch.Generator().manual_seed(seed)
    meta = {"method": method, "lora_rank": lora_rank, "arch": adapter_io.arch_numbers(a), "num_classes": classes, "weight_format": "bf16",
            "input_mean": [0.5, 0.4, 0.3], "input_std": [0.2, 0.3, 0.25], "center_crop": True, "dataset": "synthetic", "metric": "accuracy",
            "use_channel_bn": True, "normalize_visual_feature": False, "trainable_logit_scale": False, "backbone_sha256": "ab" * 32,
            "epoch": 3, "score": 61.25}
    meta.update(meta_over)
    tensors = {n: torch.randn(s, generator=g) for n, s in adapter_io.expected_tensors(meta).items()}
    tensors["channel_bn.running_var"].abs_().add_(0.5)
    tensors["channel_bn.num_batches_tracked"] = torch.tensor(12.0)
    tensors["logit_scale"] = torch.tensor(0.0)
    return meta, tensors


@pytest.mark.parametrize("method", METHODS)
def test_checkpoint_round_trip(method, tmp_path):
    meta, tensors = synthetic_ckpt(method)
    ckpt = adapter_io.make_adapter(meta, tensors)
    path = adapter_io.write_adapter(ckpt, tmp_path / "sub" / "a.pt")
    back = adapter_io.read_adapter(path)
    assert back["format"] == "pevit-adapter" and back["version"] == 1 and back["meta"] == ckpt["meta"]
    assert back["meta"]["arch"] == adapter_io.arch_numbers(ARCHS["tiny-128"]) and back["meta"]["epoch"] == 3
    assert list(back["tensors"]) == list(ckpt["tensors"])
    spec = adapter_param_spec(method, 128, 2, 4)
    assert set(back["tensors"]) == {n for n, _, _ in spec} | set(adapter_io.HEAD_TENSORS)      # frozen and dead tensors included
    for k, v in back["tensors"].items():
        assert v.dtype == torch.float32 and v.device.type == "cpu" and v.is_contiguous()
        assert torch.equal(v.view(torch.int32), tensors[k].contiguous().view(torch.int32)), k
    # the flat buffer: the trainable tower tensors in spec order, then the head
    flat = adapter_io.flat_params(back)
    want = [tensors[n].reshape(-1) for n, _, tr in spec if tr] + [tensors["layers.0.weight"].reshape(-1), tensors["layers.0.bias"]]
    assert torch.equal(flat, torch.cat(want))


def test_fingerprint_reads_three_tensors():
    g = torch.Generator().manual_seed(1)
    sd = {"visual." + k: torch.randn(4, 3, generator=g) for k in adapter_io.FINGERPRINT_KEYS}
    fp = adapter_io.backbone_fingerprint(sd)
    assert len(fp) == 64 and fp == adapter_io.backbone_fingerprint({k: v.double() for k, v in sd.items()})
    sd["visual.proj"] = sd["visual.proj"].clone(); sd["visual.proj"][0, 0] += 1e-3
    assert adapter_io.backbone_fingerprint(sd) != fp


def refused(match, fn, *a, **kw):
    with pytest.raises(adapter_io.AdapterError, match=match):
        fn(*a, **kw)


def test_every_refusal_names_its_field(tmp_path):
    meta, tensors = synthetic_ckpt("lora")
    ckpt = adapter_io.make_adapter(meta, tensors)
    arch = ARCHS["tiny-128"]
    ok = dict(method="lora", lora_rank=4, arch=arch, num_classes=7, backbone_sha256="ab" * 32)
    assert adapter_io.check_adapter(ckpt, **ok) is ckpt and adapter_io.check_adapter(ckpt, max_classes=7) is ckpt
    refused("^format", adapter_io.check_adapter, dict(ckpt, format="something-else"))
    refused("^format", adapter_io.check_adapter, [1, 2])
    refused("^version", adapter_io.check_adapter, dict(ckpt, version=2))
    refused("^method", adapter_io.check_adapter, ckpt, **dict(ok, method="kadaptation"))
    refused("^method", adapter_io.check_adapter, dict(ckpt, meta=dict(ckpt["meta"], method="prefix-tuning")))
    refused("^lora_rank", adapter_io.check_adapter, ckpt, **dict(ok, lora_rank=8))
    refused(r"^arch\.width", adapter_io.check_adapter, ckpt, **dict(ok, arch=ARCHS["tiny-256"]))
    refused(r"^arch\.patch", adapter_io.check_adapter, ckpt, **dict(ok, arch=ARCHS["tiny-n257"]))
    refused("^num_classes", adapter_io.check_adapter, ckpt, **dict(ok, num_classes=10))
    refused("^num_classes", adapter_io.check_adapter, ckpt, max_classes=6)
    refused(r"^meta\.metric", adapter_io.check_adapter, dict(ckpt, meta={k: v for k, v in ckpt["meta"].items() if k != "metric"}))
    name = "visual.transformer.resblocks.1.attn.v_proj_adapter2.weight"
    refused(f"^tensor {re.escape(name)}: missing", adapter_io.check_adapter,
            dict(ckpt, tensors={k: v for k, v in ckpt["tensors"].items() if k != name}))
    refused("^tensor optimizer.momentum: not part", adapter_io.check_adapter, dict(ckpt, tensors=dict(ckpt["tensors"], **{"optimizer.momentum": torch.zeros(3)})))
    refused("^tensor layers.0.bias: shape", adapter_io.check_adapter, dict(ckpt, tensors=dict(ckpt["tensors"], **{"layers.0.bias": torch.zeros(8)})))
    refused("^tensor layers.0.bias: must be a contiguous float32", adapter_io.check_adapter,
            dict(ckpt, tensors=dict(ckpt["tensors"], **{"layers.0.bias": torch.zeros(7, dtype=torch.float64)})))
    for bad in (float("nan"), float("inf")):
        w = ckpt["tensors"]["layers.0.weight"].clone(); w[3, 5] = bad
        refused("^tensor layers.0.weight: non-finite", adapter_io.check_adapter, dict(ckpt, tensors=dict(ckpt["tensors"], **{"layers.0.weight": w})))
    refused("^backbone_sha256", adapter_io.check_adapter, ckpt, **dict(ok, backbone_sha256="cd" * 32))
    with pytest.warns(UserWarning, match="backbone_sha256"):
        assert adapter_io.check_adapter(ckpt, strict_backbone=False, **dict(ok, backbone_sha256="cd" * 32)) is ckpt
    # a file is checked as it is read, and writing checks first
    torch.save(dict(ckpt, version=3), tmp_path / "v3.pt")
    refused("^version", adapter_io.read_adapter, tmp_path / "v3.pt")
    refused("^tensor", adapter_io.write_adapter, dict(ckpt, tensors={}), tmp_path / "never.pt")
    assert not (tmp_path / "never.pt").exists()


def test_head_switches_the_engine_does_not_compute_are_refused():
    for method in ("kadaptation", "none"):
        ckpt = adapter_io.make_adapter(*synthetic_ckpt(method))
        assert adapter_io.check_servable(ckpt) is ckpt
        refused("^use_channel_bn", adapter_io.check_servable, dict(ckpt, meta=dict(ckpt["meta"], use_channel_bn=False)))
        refused("^normalize_visual_feature", adapter_io.check_servable, dict(ckpt, meta=dict(ckpt["meta"], normalize_visual_feature=True)))
    # the linear probe multiplies its logits by exp(logit_scale): served only while that is 1
    scaled = dict(ckpt, tensors=dict(ckpt["tensors"], logit_scale=torch.tensor(2.659)))
    refused("^logit_scale", adapter_io.check_servable, scaled)


class _NotATensor:
    pass


def test_a_file_that_needs_unpickling_of_anything_else_is_refused(tmp_path):
    meta, tensors = synthetic_ckpt("adapter")
    ckpt = adapter_io.make_adapter(meta, tensors)
    ckpt["meta"]["extra"] = _NotATensor()
    torch.save(ckpt, tmp_path / "unsafe.pt")
    refused("^format: .*not a tensors-only adapter checkpoint", adapter_io.read_adapter, tmp_path / "unsafe.pt")
    (tmp_path / "garbage.pt").write_bytes(b"not a checkpoint at all")
    refused("^format", adapter_io.read_adapter, tmp_path / "garbage.pt")


# ---- where the new code lives ---------------------------------------------------------------------------------------------------
def test_serving_lives_in_modules_of_its_own():
    import inspect
    from pevit_amd import engine, engine_dp, engine_input, engine_optim, serving, text_engine, _context
    assert serving.InferenceEngine.__module__ == "pevit_amd.serving"
    assert issubclass(serving.InferenceEngine, _context.EngineContext) and issubclass(serving.InferenceEngine, engine_input.InputMixin)
    assert not issubclass(serving.InferenceEngine, engine.HipEngine) and not issubclass(engine.HipEngine, serving.InferenceEngine)
    for mod in (engine, engine_input, engine_optim, engine_dp, _context, text_engine):
        for name, obj in vars(mod).items():
            if inspect.isclass(obj) or inspect.isfunction(obj):
                assert obj.__module__ not in ("pevit_amd.serving", "pevit_amd.adapter_io"), (mod.__name__, name)
    # the state-keeping class of the new modules is the one host class; adapter_io keeps no state at all
    stateful = [n for mod in (serving, adapter_io) for n, o in vars(mod).items()
                if inspect.isclass(o) and o.__module__ == mod.__name__ and "__init__" in vars(o)]
    assert stateful == ["InferenceEngine"]


def test_the_predict_command_and_its_alias():
    import importlib
    from pevit_amd.commands import predict
    alias = importlib.import_module("vision_benchmark.commands.predict")
    assert alias.main is predict.main
    with pytest.raises(SystemExit):
        predict.main(["--model", "model.yaml"])               # --adapter is required
