"""train -> save the adapter -> load it next to a frozen tower in a context that can only infer -> predict, on the GPU.

The inference-only context (``pevit_infer_create``, pevit_amd/serving.py) runs the inference walk of ``HipEngine.predict``
instance for instance -- the same kernels on the same operands, in an arena without the transposed copies and a workspace without
the backward's slots -- so every comparison with ``HipEngine`` here is bit for bit, without a tolerance.  (One comparison is
of another kind and says so: the linear probe's cached validation runs another head kernel than ``pevit_predict``.)

Cases (tests/test_gpu_workspace.py's): tiny-128 (N = 10, H = 2: the fused delta + attention form, class-token pruning;
``max_batch`` 8), tiny-256 (N = 17, H = 4: two-kernel attention, the fused post-MLP adapter kernels; ``max_batch`` 5), tiny-n257
(N = 257: the N > 64 branch, patch 14 padding; ``max_batch`` 4); every method in bf16 and f32-verify, kadaptation / lora / none
in fp8 and fp8-act."""
import ctypes as C
import functools
import json

import pytest
import torch

from conftest import load_tiny_sd

from test_gpu_workspace import assert_flags_clear, differences, poison

pytestmark = pytest.mark.gpu

CLASSES = 10
MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
STEP = dict(lr=0.05, momentum=0.9, weight_decay=1e-3)
ARCH_BATCH = {"tiny-128": (8, 5), "tiny-256": (5, 3), "tiny-n257": (4, 3)}
METHODS = ["kadaptation", "lora", "adapter", "compacter", "none"]
CASES = [(a, m, f) for a in ARCH_BATCH for f in ("bf16", "f32-verify") for m in METHODS] + \
        [(a, m, f) for a in ARCH_BATCH for f in ("fp8", "fp8-act") for m in ("kadaptation", "lora", "none")]


@pytest.fixture(scope="module", autouse=True)
def _gpu_and_cleanup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield
    trained.cache_clear()
    backbone.cache_clear()


@functools.lru_cache(maxsize=None)
def backbone(arch_name):
    """The frozen tower tests/test_gpu_predict.py's make_engine loads"""
    from pevit_amd.synth import ARCHS, synth_state_dict
    return {k: v for k, v in synth_state_dict(ARCHS[arch_name], seed=2, text_tower=False).items() if k.startswith("visual.")}


def images_of(arch, n, seed=3):
    from test_gpu_predict import images_for
    return images_for(arch, n, seed=seed)


@functools.lru_cache(maxsize=4)
def trained(arch_name, method, weight_format, classes=CLASSES, seed=3):
    """A ``HipEngine`` with synthetic weights, non-zero adapters and non-trivial running statistics after three train steps,
    and its checkpoint."""
    from pevit_amd import adapter_io
    from test_gpu_predict import make_engine
    max_batch = ARCH_BATCH[arch_name][0]
    arch, eng = make_engine(arch_name, method, max_batch, weight_format=weight_format, classes=classes)
    rule = None
    if method == "compacter":              # (the synthetic state dict leaves the frozen rule zero)
        rule = torch.rand((4, 4, 4), generator=torch.Generator().manual_seed(11)) * 2 - 1
        eng.load_phm_rule(rule)
    eng.set_input_normalization(MEAN, STD)
    img = images_of(arch, max_batch, seed=seed)
    labels = (torch.arange(max_batch) % classes).cuda()
    for _ in range(3):
        eng.train_step(img, labels, **STEP)
    torch.cuda.synchronize()
    ckpt = adapter_io.engine_adapter_state(eng, backbone(arch_name), phm_rule=rule)
    return arch, eng, ckpt


def serving_engine(arch_name, method, weight_format, ckpts, max_classes=CLASSES, max_batch=None):
    from pevit_amd.serving import InferenceEngine
    from pevit_amd.synth import ARCHS
    inf = InferenceEngine(ARCHS[arch_name], method, max_classes, max_batch or ARCH_BATCH[arch_name][0], weight_format=weight_format)
    inf.load_backbone(backbone(arch_name))
    for name, ck in ckpts.items():
        inf.add_adapter(name, ck)
    return inf


def same_bits(got, want):
    bad = differences(got, want)
    assert not bad, bad


# ---- parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch_name,method,weight_format", CASES)
def test_predict_is_hipengine_predict_bit_for_bit(arch_name, method, weight_format, tmp_path):
    from pevit_amd import adapter_io
    arch, eng, ckpt = trained(arch_name, method, weight_format)
    path = adapter_io.write_adapter(ckpt, tmp_path / "adapter.pt")
    inf = serving_engine(arch_name, method, weight_format, {"a": path})
    assert inf.adapters() == ["a"] and 0 < inf.arena_bytes < eng.arena.numel() and 0 < inf.workspace_bytes < eng.workspace.numel()
    with pytest.raises(Exception, match="no adapter selected"):
        inf.predict(images_of(arch, 1))
    inf.use("a")
    big, odd = ARCH_BATCH[arch_name]
    for B in (big, odd, 1):
        img = images_of(arch, B, seed=20 + B)
        want = dict(zip(("logits", "features"), eng.predict(img, return_features=True)))
        got = dict(zip(("logits", "features"), inf.predict(img, return_features=True)))
        assert got["logits"].shape == (B, CLASSES) and float(got["logits"].abs().max()) > 0
        same_bits(got, want)
        same_bits({"features": inf.encode_image(img)}, {"features": want["features"]})
        assert_flags_clear(inf)


def test_uint8_input_with_the_engine_resize(tmp_path):
    arch, eng, ckpt = trained("tiny-128", "kadaptation", "bf16")
    inf = serving_engine("tiny-128", "kadaptation", "bf16", {"a": ckpt})
    inf.use("a")
    g = torch.Generator().manual_seed(8)
    exact = torch.randint(0, 256, (5, 3, 48, 48), generator=g, dtype=torch.uint8).cuda()
    native = torch.randint(0, 256, (5, 3, 60, 70), generator=g, dtype=torch.uint8).cuda()
    with pytest.raises(Exception, match="float32"):
        inf.predict(exact)                                    # uint8 before set_input_normalization
    inf.set_input_normalization(MEAN, STD)
    same_bits({"logits": inf.predict(exact)}, {"logits": eng.predict(exact)})
    for e in (eng, inf):
        e.set_input_resize(True)
    try:
        want = dict(zip(("logits", "features"), eng.predict(native, return_features=True)))
        same_bits(dict(zip(("logits", "features"), inf.predict(native, return_features=True))), want)
        # 13 native-size images on max_batch 8: two chunks through the resize staging
        many = torch.randint(0, 256, (13, 3, 60, 70), generator=g, dtype=torch.uint8).cuda()
        want = torch.cat([eng.predict(many[:8]).clone(), eng.predict(many[8:]).clone()])
        same_bits({"logits": inf.predict(many)}, {"logits": want})
    finally:
        eng.set_input_resize(False)


@pytest.mark.parametrize("weight_format", ["bf16", "fp8", "f32-verify"])
def test_encode_image_and_zeroshot_on_a_frozen_tower(weight_format):
    from test_gpu_predict import make_engine
    arch, eng = make_engine("tiny-128", "none", 8, weight_format=weight_format)
    inf = serving_engine("tiny-128", "none", weight_format, {})
    g = torch.Generator().manual_seed(4)
    text = torch.nn.functional.normalize(torch.randn((6, arch.embed_dim), generator=g)).cuda().contiguous()
    for B in (8, 5, 1):
        img = images_of(arch, B, seed=30 + B)
        same_bits({"features": inf.encode_image(img)}, {"features": eng.encode_image(img)})
        keys = ("probs", "logits", "features")
        want = dict(zip(keys, eng.zeroshot(img, text, return_logits=True, return_features=True)))
        same_bits(dict(zip(keys, inf.zeroshot(img, text, return_logits=True, return_features=True))), want)
    with pytest.raises(Exception, match="no adapter selected"):
        inf.predict(images_of(arch, 1))


# ---- chunking -------------------------------------------------------------------------------------------------------------------
def test_more_images_than_max_batch_run_in_chunks():
    arch, eng, ckpt = trained("tiny-256", "adapter", "bf16")
    inf = serving_engine("tiny-256", "adapter", "bf16", {"a": ckpt})
    inf.use("a")
    img = images_of(arch, 13, seed=41)
    parts = [inf.predict(img[lo:lo + 5], return_features=True) for lo in (0, 5, 10)]
    want = {"logits": torch.cat([p[0] for p in parts]), "features": torch.cat([p[1] for p in parts])}
    out = torch.empty((13, CLASSES), dtype=torch.float32, device="cuda")
    logits, feat = inf.predict(img, logits_out=out, return_features=True)
    assert logits is out and want["logits"].shape == (13, CLASSES)
    same_bits({"logits": logits, "features": feat}, want)
    same_bits({"features": inf.encode_image(img)}, {"features": want["features"]})
    # ... and each chunk is the training engine's predict of those rows
    same_bits({"logits": logits[5:10]}, {"logits": eng.predict(img[5:10])})


# ---- swap -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["kadaptation", "compacter"])
def test_two_resident_adapters_swap_by_pointer(method):
    arch_name = "tiny-128" if method == "kadaptation" else "tiny-256"
    arch, _, ten = trained(arch_name, method, "bf16")
    _, _, seven = trained(arch_name, method, "bf16", classes=7, seed=9)
    if method == "compacter":              # every Compacter run draws its own frozen rule: the swap must carry it
        rule = torch.rand((4, 4, 4), generator=torch.Generator().manual_seed(12)) * 2 - 1
        seven = dict(seven, tensors=dict(seven["tensors"], **{"visual.transformer.phm_rule": rule}))
    both = serving_engine(arch_name, method, "bf16", {"ten": ten, "seven": seven})
    alone = {n: serving_engine(arch_name, method, "bf16", {n: ck}) for n, ck in (("ten", ten), ("seven", seven))}
    assert both.adapters() == ["ten", "seven"]
    img = images_of(arch, ARCH_BATCH[arch_name][0], seed=50)
    want = {}
    for n, e in alone.items():
        e.use(n)
        want[n] = dict(zip(("logits", "features"), e.predict(img, return_features=True)))
    assert not torch.equal(want["ten"]["features"], want["seven"]["features"])
    for n in ("ten", "seven", "ten", "seven", "seven", "ten"):
        both.use(n)
        got = dict(zip(("logits", "features"), both.predict(img, return_features=True)))
        assert got["logits"].shape[1] == {"ten": 10, "seven": 7}[n]
        same_bits(got, want[n])
    both.drop("seven")
    assert both.adapters() == ["ten"]
    same_bits({"logits": both.predict(img)}, {"logits": want["ten"]["logits"]})
    both.drop("ten")
    with pytest.raises(Exception, match="no adapter selected"):
        both.predict(img)


def test_add_adapter_refuses_what_this_context_cannot_serve():
    from pevit_amd import adapter_io
    _, _, ckpt = trained("tiny-128", "kadaptation", "bf16")
    inf = serving_engine("tiny-128", "kadaptation", "bf16", {}, max_classes=8)
    with pytest.raises(adapter_io.AdapterError, match="^num_classes"):
        inf.add_adapter("a", ckpt)
    for arch_name, method, match in (("tiny-256", "kadaptation", r"^arch\.width"), ("tiny-128", "lora", "^method")):
        other = serving_engine(arch_name, method, "bf16", {})
        with pytest.raises(adapter_io.AdapterError, match=match):
            other.add_adapter("a", ckpt)
    inf = serving_engine("tiny-128", "kadaptation", "bf16", {})
    moved = dict(ckpt, meta=dict(ckpt["meta"], backbone_sha256="00" * 32))
    with pytest.raises(adapter_io.AdapterError, match="^backbone_sha256"):
        inf.add_adapter("a", moved)
    with pytest.warns(UserWarning, match="backbone_sha256"):
        inf.add_adapter("a", moved, strict_backbone=False)
    with pytest.raises(adapter_io.AdapterError, match="^normalize_visual_feature"):
        inf.add_adapter("b", dict(ckpt, meta=dict(ckpt["meta"], normalize_visual_feature=True)))
    assert inf.adapters() == ["a"]


# ---- self-contained under poison ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch_name,method,weight_format", [
    ("tiny-128", "kadaptation", "bf16"), ("tiny-128", "lora", "fp8"), ("tiny-128", "kadaptation", "fp8-act"), ("tiny-128", "compacter", "f32-verify"),
    ("tiny-256", "adapter", "bf16"), ("tiny-256", "compacter", "bf16"), ("tiny-256", "lora", "bf16"), ("tiny-n257", "kadaptation", "bf16"),
    ("tiny-n257", "adapter", "f32-verify"), ("tiny-n257", "none", "fp8")])
def test_every_call_is_self_contained_under_poison(arch_name, method, weight_format):
    arch, eng, ckpt = trained(arch_name, method, weight_format)
    P, Q = (serving_engine(arch_name, method, weight_format, {"a": ckpt}) for _ in range(2))
    text = torch.nn.functional.normalize(torch.randn((6, arch.embed_dim), generator=torch.Generator().manual_seed(4))).cuda().contiguous()
    for e in (P, Q):
        e.use("a")
        e.set_input_normalization(MEAN, STD)
    big, odd = ARCH_BATCH[arch_name]
    u8 = torch.randint(0, 256, (odd, 3, arch.resolution, arch.resolution), generator=torch.Generator().manual_seed(6), dtype=torch.uint8).cuda()
    calls = [("predict", lambda e, B: dict(zip(("logits", "features"), e.predict(images_of(arch, B, seed=60 + B), return_features=True)))),
             ("encode_image", lambda e, B: {"features": e.encode_image(images_of(arch, B, seed=70 + B))}),
             ("zeroshot", lambda e, B: dict(zip(("probs", "logits"), e.zeroshot(images_of(arch, B, seed=80 + B), text, return_logits=True)))),
             ("predict_u8", lambda e, B: {"logits": e.predict(u8[:min(B, odd)])})]
    for B in (big, odd, 1, big):
        for name, call in calls:
            poison(P)
            got, want = call(P, B), call(Q, B)
            bad = differences(got, want)
            assert not bad, (name, B, bad)
            assert_flags_clear(P)
    # ... and it is the training engine's answer
    img = images_of(arch, odd, seed=60 + odd)
    same_bits({"logits": P.predict(img)}, {"logits": eng.predict(img)})


@pytest.mark.parametrize("weight_format", ["fp8", "fp8-act"])
def test_fp8_loading_needs_no_workspace_scratch(weight_format):
    """A training context borrows 3 E E floats of workspace to pack wqkvT (and gives up what a forward saved there); a context
    bound for ONE image loads without touching a byte of its workspace."""
    arch, eng, ckpt = trained("tiny-256", "lora", weight_format)
    one = serving_engine("tiny-256", "lora", weight_format, {}, max_batch=1)
    poison(one)
    before = one.workspace.clone()
    one.load_backbone(backbone("tiny-256"))
    torch.cuda.synchronize()
    assert torch.equal(one.workspace, before)                 # the load did not touch the workspace at all
    one.add_adapter("a", ckpt)
    one.use("a")
    img = images_of(arch, 3, seed=90)
    want = torch.cat([eng.predict(img[i:i + 1]).clone() for i in range(3)])
    same_bits({"logits": one.predict(img)}, {"logits": want})
    assert_flags_clear(one)


# ---- everything else is refused -------------------------------------------------------------------------------------------------
def test_every_other_entry_point_is_refused_before_any_launch():
    from pevit_amd import _lib
    arch, eng, ckpt = trained("tiny-128", "kadaptation", "bf16")
    inf = serving_engine("tiny-128", "kadaptation", "bf16", {"a": ckpt})
    inf.use("a")
    inf.predict(images_of(arch, 8))
    poison(inf)
    before = inf.workspace.clone()
    lib, ctx, s = inf.lib, inf._ctx, _lib.stream_ptr()
    buf = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    p = _lib.ptr(buf)
    probe, probe_predict = _lib.PevitProbeArgs(), _lib.PevitProbePredictArgs()
    group = _lib.PevitOptimGroup()
    calls = {
        "pevit_set_params": (ctx, p, p, p, p),
        "pevit_set_optim_state": (ctx, p, p),
        "pevit_set_step_gate": (ctx, None),
        "pevit_set_external_poison": (ctx, None),
        "pevit_transformer_forward": (ctx, s, p, p, 4, 1),
        "pevit_transformer_backward": (ctx, s, p, p, 4),
        "pevit_blocks_forward": (ctx, s, p, p, 4, 1, 0, 1),
        "pevit_blocks_backward": (ctx, s, p, p, 4, 0, 1),
        "pevit_attention_forward": (ctx, s, 0, p, p, 4, 1, None, 1),
        "pevit_attention_backward": (ctx, s, 0, p, p, 4),
        "pevit_visual_forward": (ctx, s, p, p, 4, 1),
        "pevit_visual_forward_u8": (ctx, s, p, p, 4, 1),
        "pevit_visual_backward": (ctx, s, p, 4),
        "pevit_visual_backward_part": (ctx, s, p, 4, 2, 0),
        "pevit_head_forward_backward": (ctx, s, p, p, p, p, 1, p, p, p, 4),
        "pevit_head_forward_backward_bce": (ctx, s, p, p, p, p, 1, p, p, p, 4),
        "pevit_train_forward_backward": (ctx, s, p, p, p, p, 1, p, p, 4),
        "pevit_train_forward_backward_u8": (ctx, s, p, p, p, p, 1, p, p, 4),
        "pevit_train_forward_backward_bce": (ctx, s, p, p, p, p, 1, p, p, 4),
        "pevit_train_forward_backward_bce_u8": (ctx, s, p, p, p, p, 1, p, p, 4),
        "pevit_zero_grads": (ctx, s),
        "pevit_sgd_step": (ctx, s, 0.1, 0.9, 0.0, 1.0, 1),
        "pevit_optim_step": (ctx, s, 0, C.byref(group), 1, 1, 1.0, 1),
        "pevit_probe_step": (ctx, s, C.byref(probe)),
        "pevit_probe_predict": (ctx, s, C.byref(probe_predict)),
        "pevit_encode_text": (ctx, s, p, p, 4),
    }
    # every entry of the C ABI that takes a context is either served, a size / status / tune / profile query, or in this list
    served = {"pevit_ctx_destroy", "pevit_bind", "pevit_load_block", "pevit_load_stem", "pevit_load_phm_rule", "pevit_set_input_norm",
              "pevit_set_infer_params", "pevit_predict", "pevit_predict_u8", "pevit_encode_image", "pevit_encode_image_u8",
              "pevit_zeroshot", "pevit_zeroshot_u8", "pevit_arena_bytes", "pevit_workspace_bytes", "pevit_workspace_state_bytes",
              "pevit_num_tower_params", "pevit_num_params", "pevit_param_layer_offset", "pevit_param_grad_mask", "pevit_tune",
              "pevit_streamk_error", "pevit_streamk_status", "pevit_profile_begin", "pevit_profile_end", "pevit_profile_launch",
              "pevit_profile_launch_bytes", "pevit_load_text_stem"}
    takes_ctx = {n for n in _lib.SIGNATURES if not n.startswith(("pevit_op_", "pevit_debug_", "pevit_ar_", "pevit_resize_"))} - \
        {"pevit_last_error", "pevit_version", "pevit_ctx_create", "pevit_infer_create", "pevit_text_create", "pevit_allreduce_flat"}
    assert takes_ctx == served | set(calls), takes_ctx ^ (served | set(calls))
    for name, args in calls.items():
        assert getattr(lib, name)(*args) != 0, name
        assert b"inference-only context" in lib.pevit_last_error(), (name, lib.pevit_last_error())
    torch.cuda.synchronize()
    assert torch.equal(inf.workspace, before)                 # flag words zero, every other byte still poison: nothing was launched
    assert not bool(buf.any())
    assert_flags_clear(inf)
    assert lib.pevit_load_text_stem(ctx, s, p, p, p, p, p) != 0         # (a text context's loader: refused as on any image context)
    same_bits({"logits": inf.predict(images_of(arch, 8))}, {"logits": eng.predict(images_of(arch, 8))})


# ---- back into training, and the harness ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_ckpt(tmp_path_factory):
    p = tmp_path_factory.mktemp("ckpt") / "tiny.pt"
    torch.save(load_tiny_sd(), p)
    return p


@pytest.mark.parametrize("method", ["kadaptation", "compacter"])
def test_load_adapter_puts_a_checkpoint_back_into_a_classifier(method, tiny_ckpt, tmp_path):
    from conftest import load_golden
    from pevit_amd import adapter_io
    from test_gpu_mirror import OneBatch, seeded_classifier
    meta, t = load_golden("tiny_" + method)
    mod, cfg, clf = seeded_classifier(method, tiny_ckpt, meta, t)
    crit, opt = torch.nn.CrossEntropyLoss().cuda(0), mod.build_optimizer(cfg, clf)
    mod.train_one(OneBatch(t["images"], t["labels"], 3), clf, crit, opt, 0, cfg)
    clf.eval()
    path = adapter_io.save_adapter(clf, tmp_path / "a.pt", **adapter_io.config_meta(cfg), epoch=0)
    saved = adapter_io.read_adapter(path)
    assert saved["meta"]["method"] == method and saved["meta"]["dataset"] == cfg.DATASET.DATASET and saved["meta"]["epoch"] == 0
    assert float(saved["tensors"]["channel_bn.num_batches_tracked"]) == 3.0
    images = t["images"].cuda()
    want = clf.fused_predict(images).clone()
    state = {n: p.detach().cpu().clone() for n, p in clf.named_parameters() if p.requires_grad or "phm_rule" in n}
    bn = {k: v.detach().cpu().clone() for k, v in clf.channel_bn.state_dict().items()}
    del clf, opt
    _, _, fresh = seeded_classifier(method, tiny_ckpt, meta, t)
    with pytest.raises(adapter_io.AdapterError, match="^num_classes"):
        adapter_io.load_adapter(fresh, dict(saved, meta=dict(saved["meta"], num_classes=3),
                                            tensors=dict(saved["tensors"], **{"layers.0.weight": torch.zeros(3, 64), "layers.0.bias": torch.zeros(3)})))
    adapter_io.load_adapter(fresh, path)
    got = {n: p.detach().cpu() for n, p in fresh.named_parameters() if p.requires_grad or "phm_rule" in n}
    same_bits(got, state)
    got_bn = {k: v.detach().cpu() for k, v in fresh.channel_bn.state_dict().items()}
    assert list(got_bn) == list(bn) and all(torch.equal(got_bn[k], bn[k]) for k in bn) and int(got_bn["num_batches_tracked"]) == 3
    fresh.eval()
    same_bits({"logits": fresh.fused_predict(images)}, {"logits": want})          # the engine holds them too (Compacter: its rule)
    same_bits(adapter_io.adapter_state(fresh)["tensors"], saved["tensors"])


def test_the_harness_saves_the_best_adapter_and_the_command_reproduces_its_score(tiny_ckpt, tmp_path, monkeypatch):
    from pevit_amd import adapter_io
    from pevit_amd.commands import _finetune, kronecker_adaptation_clip as train_cmd, predict as predict_cmd
    from pevit_amd.config import default_config
    from pevit_amd.evaluation import _harness
    _harness._BACKBONES.clear()
    model = tmp_path / "model.yaml"
    model.write_text(f"MODEL:\n  NAME: '{tiny_ckpt}'\n  SPEC:\n    EMBED_DIM: 64\nTRAIN:\n  END_EPOCH: 1\n  EXTRA_FINAL_TRAIN_EPOCH: 1\n"
                     "  NESTEROV: false\n  WD: 0.\nTEST:\n  METRIC: 'accuracy'\n")
    opts = ["DATASET.DATASET", "synthetic", "DATASET.NUM_CLASSES", "5", "OUTPUT_DIR", str(tmp_path / "out"), "TRAIN.IMAGE_SIZE", "[48, 48]",
            "DATASET.SYNTHETIC_SIZES", "(40, 10)"]
    monkeypatch.setattr(_finetune, "config", default_config())
    acc, info = train_cmd.main(["--model", str(model), "--no-tuning", "True", "--lr", "0.01", "--l2", "1e-6"] + opts +
                               ["TRAIN.SAVE_ADAPTER", "best"])
    path = tmp_path / "out" / "adapter_synthetic_kadaptation.pt"
    assert info["adapter_file"] == str(path) and path.is_file() and acc > 0
    saved = adapter_io.read_adapter(path)
    assert saved["meta"]["score"] == acc and saved["meta"]["epoch"] in (0, 1) and saved["meta"]["num_classes"] == 5
    assert saved["meta"]["input_mean"] == default_config().INPUT.MEAN and saved["meta"]["metric"] == "accuracy"
    monkeypatch.setattr(predict_cmd, "config", default_config())
    result, probs, metric = predict_cmd.main(["--model", str(model), "--adapter", str(path)] + opts)
    assert metric == "accuracy" and result == acc
    assert probs.shape == (10, 5) and probs.dtype == info["best_logits"].dtype
    assert (probs.view("int32") == info["best_logits"].view("int32")).all()
    j = json.load(open(tmp_path / "out" / "predictions" / "predict_kadaptation" / "synthetic.json"))
    assert set(j) == {"model_name", "dataset_name", "num_trainable_params", "num_params", "num_visual_params",
                      "num_backbone_params", "n_shot", "rnd_seeds", "predictions"}
    assert len(j["predictions"][0]) == 10 and j["num_trainable_params"] == info["n_trainable_params"]
    _harness._BACKBONES.clear()


def test_save_adapter_off_by_default_and_refused_values(tiny_ckpt, tmp_path, monkeypatch):
    from pevit_amd.commands import _finetune, kronecker_adaptation_clip as train_cmd
    from pevit_amd.config import default_config
    from pevit_amd.evaluation import _harness
    _harness._BACKBONES.clear()
    model = tmp_path / "model.yaml"
    model.write_text(f"MODEL:\n  NAME: '{tiny_ckpt}'\n  SPEC:\n    EMBED_DIM: 64\nTRAIN:\n  END_EPOCH: 1\n  NESTEROV: false\n  WD: 0.\n")
    opts = ["--model", str(model), "--no-tuning", "True", "--lr", "0.01", "DATASET.DATASET", "synthetic", "DATASET.NUM_CLASSES", "5",
            "OUTPUT_DIR", str(tmp_path / "out"), "TRAIN.IMAGE_SIZE", "[48, 48]", "DATASET.SYNTHETIC_SIZES", "(40, 10)"]
    monkeypatch.setattr(_finetune, "config", default_config())
    _, info = train_cmd.main(opts)
    assert "adapter_file" not in info and not list((tmp_path / "out").glob("adapter_*"))
    monkeypatch.setattr(_finetune, "config", default_config())
    _, info = train_cmd.main(opts + ["TRAIN.SAVE_ADAPTER", "last"])
    assert info["adapter_file"].endswith("adapter_synthetic_kadaptation.pt")
    monkeypatch.setattr(_finetune, "config", default_config())
    with pytest.raises(ValueError, match="SAVE_ADAPTER"):
        train_cmd.main(opts + ["TRAIN.SAVE_ADAPTER", "every-epoch"])
    _harness._BACKBONES.clear()


def test_the_linear_probe_saves_its_head_and_the_context_serves_it(tiny_ckpt, tmp_path):
    """Method "none" with a head is the linear probe's product.  Its cached validation scores rows with ``pevit_probe_predict``,
    the serving context with the head of ``pevit_predict``: the same tower bits through two f32 head kernels, so the
    probabilities agree to the rounding of a D = 64 term f32 sum (64 * 2^-23 * sum |w x| < 1e-4 for sums below 10), not bit for bit."""
    import numpy as np
    from test_mirror_api import tiny_config
    from pevit_amd import adapter_io
    from pevit_amd.commands import predict as predict_cmd
    from pevit_amd.evaluation import _harness as h, full_model_finetune as fm
    from pevit_amd.evaluation.dataloader import construct_dataloader
    cfg = tiny_config(tiny_ckpt, classes=5)
    cfg.DATASET.DATASET, cfg.DATASET.SYNTHETIC_SIZES, cfg.DATASET.LOADER_BATCH_SIZE = "synthetic", (40, 10), 16
    cfg.TRAIN.IMAGE_SIZE = [48, 48]
    cfg.TRAIN.FREEZE_IMAGE_BACKBONE, cfg.TRAIN.END_EPOCH, cfg.TRAIN.LR = True, 2, 0.01
    cfg.TRAIN.SAVE_ADAPTER, cfg.OUTPUT_DIR, cfg.GPUS = "best", str(tmp_path), (0,)
    fm.clear_feature_cache()
    h._BACKBONES.clear()
    train, _, test = construct_dataloader(cfg)
    best, info = fm.train_task(train, test, cfg)
    assert info["adapter_file"] == str(tmp_path / "adapter_synthetic_none.pt") and best > 0
    ckpt = adapter_io.read_adapter(info["adapter_file"])
    assert ckpt["meta"]["method"] == "none" and ckpt["meta"]["score"] == best and float(ckpt["tensors"]["logit_scale"]) == 0.0
    assert set(ckpt["tensors"]) == set(adapter_io.HEAD_TENSORS)
    eng = predict_cmd.build_engine(cfg, ckpt, load_tiny_sd())
    _, probs, _ = predict_cmd.score(cfg, eng)
    err = float(np.abs(probs - info["best_logits"]).max())
    print(f"probe validation vs served adapter: max |p - p'| {err:.3e} (gate 1e-4)")
    assert probs.shape == (10, 5) and err < 1e-4
    fm.clear_feature_cache()
    h._BACKBONES.clear()
