"""The inference path: images -> logits in one engine call (``pevit_predict``), and the kernel forms it is made of.

Every kernel form that stores nothing for a backward pass -- the GELU-only c_fc epilogue, the attention kernels without the
log-sum-exp (and, fused with the adapter delta, without the q' / v' write-back), LayerNorm without its statistics -- must give the
BITS of its training form, on every kernel family the planner can pick; ``HipEngine.predict`` must give the bits of the existing
route ``visual_forward(save=False)`` + the forward-only head, move nothing but its outputs, and agree with the CPU oracle within
the gate the validation test of tests/test_gpu_mirror.py uses (LOGIT_TOL of tests/test_gpu_tower.py: bf16 operands, f32
accumulation).  ``validate()`` goes through it whenever that is exactly the module's forward.
"""
import ctypes as C
import os

import pytest
import torch

from conftest import golden_param_dict, load_golden, max_rel

pytestmark = pytest.mark.gpu

EPI_BIAS_GELU, EPI_BIAS_GELU_ONLY = 2, 14


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


def rnd(*shape, scale=1.0, seed=0, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


# ---- 1. the GELU-only epilogue ---------------------------------------------------------------------------------------------------
# (M, N, K, kernel family of the bf16 product: 1 = 4-wave tile, 2 = staggered 8-wave tile -- the two the planner has for c_fc, whose
# K = E never reaches the few-row split-K kernel and whose epilogue has no k-split form)
GEMM_SHAPES = [(20, 512, 128, 1), (85, 1024, 256, 1), (6400, 3072, 768, 2)]


def _nan16(M, N):
    return torch.full((M, N), float("nan"), dtype=torch.bfloat16, device="cuda")


@pytest.mark.parametrize("M,N,K,family", GEMM_SHAPES)
def test_gelu_only_epilogue_bf16(lib, M, N, K, family):
    A = rnd(M, K, seed=1, dtype=torch.bfloat16)
    B = rnd(N, K, seed=2, scale=0.08, dtype=torch.bfloat16)
    bias = rnd(N, seed=3, scale=0.1)
    h, g, g2 = _nan16(M, N), _nan16(M, N), _nan16(M, N)

    def run(epi, outb, outb2):
        ok(lib, lib.pevit_op_gemm(S(), epi, P(A), K, P(B), K, N, M, N, K, P(bias), None, 0, None, 0, P(outb), N, P(outb2), N,
                                  None, 0, 0, 0, 0, 0))
        torch.cuda.synchronize()
        return lib.pevit_debug_last_gemm_path()
    assert run(EPI_BIAS_GELU, h, g) == family
    assert run(EPI_BIAS_GELU_ONLY, None, g2) == family
    assert torch.isfinite(g.float()).all() and float(g.float().abs().max()) > 0
    assert torch.equal(g2, g)


@pytest.mark.parametrize("M,N,K,_family", GEMM_SHAPES)
def test_gelu_only_epilogue_fp8_weights_and_fp8_activations(lib, M, N, K, _family):
    from test_gpu_fp8 import quant
    W = rnd(N, K, seed=2, scale=0.05) * torch.logspace(-1, 1, N, device="cuda")[:, None]
    bias = rnd(N, seed=3, scale=0.1)
    codes, scales, _ = quant(lib, W)
    # fp8 weights, bf16 activations
    A = rnd(M, K, seed=1, dtype=torch.bfloat16)
    h, g, g2 = _nan16(M, N), _nan16(M, N), _nan16(M, N)

    def run_w8(epi, outb, outb2):
        ok(lib, lib.pevit_op_gemm_fp8(S(), epi, P(A), K, P(codes), K, codes.shape[0], P(scales), None, M, N, K, P(bias), None, 0,
                                      None, 0, P(outb), N, P(outb2), N, None, 0, 0, 0, 0, 0))
        torch.cuda.synchronize()
        return lib.pevit_debug_last_gemm_path()
    assert run_w8(EPI_BIAS_GELU, h, g) == run_w8(EPI_BIAS_GELU_ONLY, None, g2)
    assert float(g.float().abs().max()) > 0 and torch.equal(g2, g)
    # fp8 x fp8: the activation leaves as bf16 (out2_fp8 = 0) or as k-permuted e4m3 codes (1)
    acodes = torch.zeros((M, K), dtype=torch.uint8, device="cuda")
    ok(lib, lib.pevit_op_cast_fp8(S(), P(rnd(M, K, seed=4) * 1.5), P(acodes), M, K))
    for out2_fp8 in (0, 1):
        def buf():
            return torch.full((M, N), 0x55, dtype=torch.uint8, device="cuda") if out2_fp8 else _nan16(M, N)

        def run_a8(epi, outb, outb2):
            ok(lib, lib.pevit_op_gemm_f8a(S(), epi, P(acodes), K, P(codes), K, codes.shape[0], P(scales), M, N, K, P(bias), None, 0,
                                          None, 0, P(outb), N, P(outb2), N, out2_fp8, 0, 0, 0, 0))
            torch.cuda.synchronize()
            return lib.pevit_debug_last_gemm_path()
        g, g2 = buf(), buf()
        assert run_a8(EPI_BIAS_GELU, _nan16(M, N), g) == 2 and run_a8(EPI_BIAS_GELU_ONLY, None, g2) == 2
        assert torch.equal(g2, g)
        assert not torch.equal(g, buf())                       # ... and was written


# ---- 2. attention without what only a backward pass reads -----------------------------------------------------------------------
@pytest.mark.parametrize("Bt,H,N", [(2, 2, 10), (3, 12, 50), (5, 12, 50)])
def test_fused_delta_attention_without_the_write_back(lib, Bt, H, N):
    """(2, 2, 10): B*H = 4 heads, a partial run of the six-head workgroup, on the generic instance; H = 12, N = 50: the compile-time
    <12, 50> instance, B*H a multiple of six (3) and not (5: the last run starts inside an image)."""
    from test_gpu_ops import _flat_case
    E = H * 64
    _, T, t, q32, bias, _, _ = _flat_case(Bt, N, E, seed=40)
    assert lib.pevit_op_attn_delta_hpw(Bt, H, N) == 6
    q = rnd(Bt * H, N, 64, seed=41, scale=0.35, dtype=torch.bfloat16)
    k = rnd(Bt * H, N, 64, seed=42, dtype=torch.bfloat16)
    v = rnd(Bt * H, N, 64, seed=43, dtype=torch.bfloat16)
    q16 = q32.bfloat16()
    q1, v1 = q.clone(), v.clone()
    out1 = torch.zeros((T, E), dtype=torch.bfloat16, device="cuda"); lse1 = torch.zeros((Bt * H, N), device="cuda")
    ok(lib, lib.pevit_op_attn_fwd_delta(S(), P(q1), P(k), P(v1), P(t), P(q16), P(bias), 160.0, P(out1), E, P(lse1), Bt, H, N))
    q2, v2 = q.clone(), v.clone()
    out2 = torch.zeros_like(out1)
    ok(lib, lib.pevit_op_attn_fwd_delta(S(), P(q2), P(k), P(v2), P(t), P(q16), P(bias), 160.0, P(out2), E, None, Bt, H, N))
    torch.cuda.synchronize()
    assert not torch.equal(q1, q) and not torch.equal(v1, v)       # the saving form rewrote them: the delta is no no-op here
    assert torch.equal(q2, q) and torch.equal(v2, v)               # the inference form only read them
    assert float(out1.float().abs().max()) > 0 and torch.equal(out2, out1)


@pytest.mark.parametrize("Bt,H,N", [(2, 4, 17), (1, 2, 197), (1, 2, 257)])
def test_attention_forward_without_lse(lib, Bt, H, N):
    E = H * 64
    q = rnd(Bt * H, N, 64, seed=1, scale=0.35, dtype=torch.bfloat16)
    k = rnd(Bt * H, N, 64, seed=2, dtype=torch.bfloat16)
    v = rnd(Bt * H, N, 64, seed=3, dtype=torch.bfloat16)
    out1 = torch.zeros((Bt * N, E), dtype=torch.bfloat16, device="cuda"); out2 = torch.zeros_like(out1)
    lse = torch.zeros((Bt * H, N), device="cuda")
    ok(lib, lib.pevit_op_attn_fwd(S(), P(q), P(k), P(v), P(out1), E, P(lse), Bt, H, N))
    ok(lib, lib.pevit_op_attn_fwd(S(), P(q), P(k), P(v), P(out2), E, None, Bt, H, N))
    torch.cuda.synchronize()
    assert float(out1.float().abs().max()) > 0 and torch.equal(out2, out1)


# ---- 3. LayerNorm without statistics --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,E", [(7, 128), (20, 768), (5, 1024)])
def test_layernorm_forward_without_statistics(lib, rows, E):
    x = rnd(rows, E, seed=1, scale=2.0) + 0.5
    g = 1 + rnd(E, seed=2, scale=0.2); b = rnd(E, seed=3, scale=0.2)
    y1 = torch.zeros((rows, E), dtype=torch.bfloat16, device="cuda"); y2 = torch.zeros_like(y1)
    mean = torch.zeros(rows, device="cuda"); rstd = torch.zeros(rows, device="cuda")
    ok(lib, lib.pevit_op_ln_fwd(S(), P(x), P(g), P(b), rows, E, P(y1), None, P(mean), P(rstd)))
    ok(lib, lib.pevit_op_ln_fwd(S(), P(x), P(g), P(b), rows, E, P(y2), None, None, None))
    torch.cuda.synchronize()
    assert float(y1.float().abs().max()) > 0 and torch.equal(y2, y1)


# ---- 4. predict == the existing route, bit for bit ------------------------------------------------------------------------------
def make_engine(arch_name, method, max_batch, weight_format="bf16", classes=10):
    """A synthetic tower with random NON-ZERO adapters (the reference initialisation zeroes the Kronecker factors), a random head and
    random running statistics with variance above 0.5."""
    from pevit_amd.engine import HipEngine, adapter_param_spec
    from pevit_amd.synth import ARCHS, randomize_adapters, synth_state_dict
    arch = ARCHS[arch_name]
    sd = {k: v for k, v in synth_state_dict(arch, seed=2, text_tower=False).items() if k.startswith("visual.")}
    ad = [(n, torch.zeros(s)) for n, s, _ in adapter_param_spec(method, arch.width, arch.layers)]
    randomize_adapters(ad, seed=3)
    sd.update(dict(ad))
    eng = HipEngine(arch, method, classes, max_batch, weight_format=weight_format)
    eng.load_state_dict(sd)
    g = torch.Generator().manual_seed(5)
    D = arch.embed_dim
    v = eng.param_views()
    with torch.no_grad():
        v["layers.0.weight"].copy_(((torch.rand((classes, D), generator=g) * 2 - 1) / D ** 0.5).cuda())
        v["layers.0.bias"].copy_(((torch.rand((classes,), generator=g) * 2 - 1) / D ** 0.5).cuda())
        eng.running_mean.copy_((torch.randn(D, generator=g) * 0.3).cuda())
        eng.running_var.copy_((0.5 + torch.rand(D, generator=g)).cuda())
    return arch, eng


def images_for(arch, B, seed=3):
    from pevit_amd.synth import synth_batch
    return synth_batch(B, arch.resolution, 10, seed_img=seed, seed_lbl=seed + 1)[0].cuda()


def existing_route(eng, img):
    feat = eng.visual_forward(img, save=False)
    return eng.head_forward_backward(feat, None, bn_training=False)[0], feat


def check_predict_equals_existing_route(eng, img):
    want, want_feat = existing_route(eng, img)
    got, feat = eng.predict(img, return_features=True)
    torch.cuda.synchronize()
    assert got.shape == (img.shape[0], eng.num_classes) and torch.isfinite(got).all() and float(got.abs().max()) > 0
    assert torch.equal(got, want)
    assert torch.equal(feat, want_feat)
    assert torch.equal(eng.predict(img), want)


# tiny-128 (H = 2, N = 10) takes the fused delta form, tiny-256 (H = 4, N = 17) the two-kernel form; tiny-128 runs the post-MLP
# adapters as separate launches, tiny-256 on the fused adapter kernel
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("arch_name", ["tiny-128", "tiny-256"])
@pytest.mark.parametrize("method", ["kadaptation", "lora", "adapter", "compacter", "none"])
def test_predict_equals_visual_forward_plus_head(lib, method, arch_name, B):
    arch, eng = make_engine(arch_name, method, 5)
    assert (lib.pevit_op_attn_delta_hpw(B, arch.heads, arch.tokens) == 6) == (arch_name == "tiny-128")
    check_predict_equals_existing_route(eng, images_for(arch, B))


@pytest.mark.parametrize("arch_name,method,B", [("tiny-n197", "kadaptation", 2), ("tiny-n257", "kadaptation", 2),
                                                 ("ViT-B/32-2L", "kadaptation", 3), ("ViT-B/32-2L", "lora", 3)])
def test_predict_on_the_other_attention_families_and_with_class_token_pruning(arch_name, method, B):
    """N = 197 / 257: the mid and large attention instances.  ViT-B/32-2L: the <12, 50> fused delta instance, and the last block
    after its attention core on the class-token rows only."""
    arch, eng = make_engine(arch_name, method, B)
    check_predict_equals_existing_route(eng, images_for(arch, B))


@pytest.mark.parametrize("weight_format,method", [("bf16", "kadaptation"), ("fp8", "kadaptation"), ("fp8-act", "kadaptation"),
                                                   ("f32-verify", "kadaptation"), ("f32-verify", "adapter"), ("fp8", "none")])
def test_predict_in_every_weight_format(weight_format, method):
    arch, eng = make_engine("tiny-256", method, 5, weight_format=weight_format)
    check_predict_equals_existing_route(eng, images_for(arch, 5))


def test_predict_from_uint8_pixels():
    arch, eng = make_engine("tiny-128", "kadaptation", 4)
    mean, std = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
    g = torch.Generator().manual_seed(11)
    u8 = torch.randint(0, 256, (4, 3, arch.resolution, arch.resolution), generator=g, dtype=torch.uint8).cuda()
    from pevit_amd import _lib
    with pytest.raises(_lib.PevitError):
        eng.predict(u8)                                    # no preprocessing constants yet
    eng.set_input_normalization(mean, std)
    m = torch.tensor(mean, device="cuda").view(1, 3, 1, 1); s = torch.tensor(std, device="cuda").view(1, 3, 1, 1)
    f32 = ((u8.float() / 255 - m) / s).contiguous()
    a, b = eng.predict(u8), eng.predict(f32)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and float(a.abs().max()) > 0
    out = torch.zeros_like(a)
    assert eng.predict(u8, logits_out=out) is out and torch.equal(out, a)


# ---- 5. nothing else moves ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["kadaptation", "adapter"])
def test_predict_moves_nothing_but_its_outputs(method):
    from pevit_amd import _lib
    from pevit_amd.synth import synth_batch
    arch, eng = make_engine("tiny-256", method, 6)
    _, twin = make_engine("tiny-256", method, 6)
    images, labels = synth_batch(6, arch.resolution, 10, seed_img=3, seed_lbl=4)
    images, labels = images.cuda(), labels.cuda()
    step = dict(lr=0.05, momentum=0.9, weight_decay=1e-3)
    for e in (eng, twin):
        e.train_step(images, labels, **step)
    state = lambda e: [t.clone() for t in (e.params, e.grads, e.momentum, e.running_mean, e.running_var)]
    before = state(eng)
    assert float(eng.grads.abs().max()) > 0 and float(eng.momentum.abs().max()) > 0
    first = eng.predict(images[:3])
    again = eng.predict(images[:3])
    torch.cuda.synchronize()
    assert torch.equal(first, again)
    for a, b in zip(before, state(eng)):
        assert torch.equal(a, b)
    # like every forward, predict leaves no saved forward behind
    eng.visual_forward(images, save=True)
    eng.predict(images)
    with pytest.raises(_lib.PevitError):
        eng.visual_backward(torch.ones((6, arch.embed_dim), device="cuda"))
    # train_step, predict, train_step == train_step, train_step
    l1, loss1 = eng.train_step(images, labels, **step)
    l2, loss2 = twin.train_step(images, labels, **step)
    torch.cuda.synchronize()
    assert torch.equal(l1, l2) and float(loss1) == float(loss2)
    for a, b in zip(state(eng), state(twin)):
        assert torch.equal(a, b)


# ---- 6. against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tiny_kadaptation", "tiny_adapter"])
def test_predict_matches_the_cpu_oracle(case):
    from oracle import ref_cpu
    from test_gpu_tower import LOGIT_TOL, make_engine as fixture_engine
    meta, t = load_golden(case)
    eng, sd = fixture_engine(meta, t)
    g = torch.Generator().manual_seed(9)
    D = eng.arch.embed_dim
    rm, rv = torch.randn(D, generator=g) * 0.3, 0.5 + torch.rand(D, generator=g)
    eng.running_mean.copy_(rm.cuda()); eng.running_var.copy_(rv.cuda())
    got = eng.predict(t["images"].cuda())
    with torch.no_grad():
        feat = ref_cpu.visual_forward(t["images"], {k: v.float() for k, v in sd.items()}, meta["method"])
        ref = ((feat - rm) / torch.sqrt(rv + 1e-5)) @ t["head_w"].float().T + t["head_b"].float()
    err = max_rel(got.cpu(), ref)
    print(f"{case}: predict vs oracle max_rel {err:.3e} (gate {LOGIT_TOL})")
    assert err < LOGIT_TOL


# ---- 7. the harness -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    from conftest import load_tiny_sd
    p = tmp_path_factory.mktemp("ckpt") / "tiny.pt"
    torch.save(load_tiny_sd(), p)
    return p


def _spy(clf):
    calls = []
    real = clf.fused_predict

    def spy(images):
        out = real(images)
        calls.append(out)
        return out
    clf.fused_predict = spy
    return calls


def test_validate_goes_through_fused_predict(ckpt):
    from test_gpu_mirror import OneBatch, seeded_classifier
    meta, t = load_golden("tiny_kadaptation")
    mod, cfg, clf = seeded_classifier("kadaptation", ckpt, meta, t)
    crit = torch.nn.CrossEntropyLoss().cuda(0)
    opt = mod.build_optimizer(cfg, clf)
    assert not clf.can_fuse_eval()                                  # a fresh Classifier is in train mode
    mod.train_one(OneBatch(t["images"], t["labels"], 1), clf, crit, opt, 0, cfg)
    calls = _spy(clf)
    loader = OneBatch(t["images"], t["labels"], 2)
    score, probs = mod.validate(loader, clf, crit, 0, cfg, return_logits=True)
    assert len(calls) == 2 and not clf.training and clf.can_fuse_eval() and clf.can_fuse_eval(t["images"].cuda())
    assert not clf.can_fuse_eval(t["images"]) and not clf.can_fuse_eval(t["images"].cuda().half())
    with torch.no_grad():
        want = clf(t["images"].cuda())
    err = max_rel(calls[0].cpu(), want.cpu())
    print(f"fused_predict vs clf(images) in eval mode: max_rel {err:.3e} (gate 1e-5)")
    assert err < 1e-5                                               # the same tower bits; the f32 head by the engine vs by torch
    clf.can_fuse_eval = lambda *_: False
    score2, probs2 = mod.validate(loader, clf, crit, 0, cfg, return_logits=True)
    assert len(calls) == 2 and score2 == score
    assert max_rel(torch.from_numpy(probs), torch.from_numpy(probs2)) < 1e-5


@pytest.mark.parametrize("why", ["NORMALIZE_VISUAL_FEATURE", "USE_CHANNEL_BN", "train mode"])
def test_validate_keeps_the_module_route_where_predict_is_not_the_forward(why, ckpt):
    from test_gpu_mirror import OneBatch, seeded_classifier
    meta, t = load_golden("tiny_kadaptation")
    over = {"NORMALIZE_VISUAL_FEATURE": {"NORMALIZE_VISUAL_FEATURE": True}, "USE_CHANNEL_BN": {"USE_CHANNEL_BN": False}}.get(why, {})
    mod, cfg, clf = seeded_classifier("kadaptation", ckpt, meta, t, **over)
    crit = torch.nn.CrossEntropyLoss().cuda(0)
    images = t["images"].cuda()
    if why == "train mode":
        assert clf.training and not clf.can_fuse_eval() and not clf.can_fuse_eval(images)
        clf.eval()
        assert clf.can_fuse_eval(images)
        clf.channel_bn.train()                                      # batch statistics again: not what predict computes
        assert not clf.can_fuse_eval(images)
        return                                                      # (validate() itself puts the module into eval mode)
    clf.eval()
    assert not clf.can_fuse_eval() and not clf.can_fuse_eval(images)
    calls = _spy(clf)
    _, probs = mod.validate(OneBatch(t["images"], t["labels"], 1), clf, crit, 0, cfg, return_logits=True)
    assert not calls
    with torch.no_grad():
        want = clf(images).softmax(-1)
    assert torch.equal(torch.from_numpy(probs), want.cpu())


# ---- 8. data parallel: predict behind a pipelined step --------------------------------------------------------------------------
def test_predict_right_behind_a_pipelined_step_sees_the_finished_update():
    """The pipelined DP schedule leaves the all-reduce and the SGD kernel of a step on a second stream; predict must wait for them
    (dp_flush) like every other reader of the parameters.  One rank, in process, as
    tests/test_gpu_tower.py::test_state_reads_right_behind_a_pipelined_step_see_the_finished_update drives that schedule."""
    import torch.distributed as dist
    from test_gpu_tower import make_engine as fixture_engine
    meta, t = load_golden("tiny_kadaptation")
    images, labels = t["images"].cuda(), t["labels"].cuda()
    eng_a, _ = fixture_engine(meta, t)
    eng_b, _ = fixture_engine(meta, t)
    own_group = not dist.is_initialized()
    if own_group:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29536")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        for step in range(3):
            eng_a.forward_backward_dp(images, labels, mode="single"); eng_a.sgd_step(0.01, 0.9, 1e-4, 1.0)
            eng_b._train_step_pipelined(images, labels, 0.01, 0.9, 1e-4, True, None, 1, False, None, None)
            got = eng_b.predict(images)                            # no synchronize, no explicit flush
            want = eng_a.predict(images)
            assert torch.equal(got, want), step
        assert eng_b._pipe is not None and not eng_b._pipe["open"]                 # predict flushed
    finally:
        if own_group:
            dist.destroy_process_group()
