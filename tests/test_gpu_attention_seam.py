"""MultiheadAttention.forward of resblocks[i].attn on the engine (pevit_attention_forward / _backward, attn_probs.hip), on the GPU:

  * the probabilities kernel against torch softmax(q k^T) on the same bf16 q and k, with lse from the attention forward kernel;
  * the seam's output, weights, input gradient and adapter gradients, every PEFT method, in the f32-class verification mode
    against the f32 oracle (oracle/ref_cpu.py) and in the production bf16 mode against the rounding-point emulation
    (oracle/emul_bf16.py);
  * consistency with the block seam: x + attn(ln_1(x)) followed by the MLP half reproduces resblocks[i](x);
  * the saved-state rules (a block forward in between makes the seam's backward raise, and the reverse) and the refusal of a
    gradient through the weights;
  * fp8 weights: bit-identical to bf16 weights on the de-quantised values.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import load_tiny_sd, rel_err

pytestmark = pytest.mark.gpu
METHODS = ["kadaptation", "lora", "adapter", "compacter"]

# f32-class verification mode: the stated gate of BASELINE.md section 3 is 2e-2; every contraction is f32 there, so the output,
# the weights and dx are held 20x tighter, the adapter gradients (chained through the Kronecker / low-rank factors) at the gate
F32_Y_TOL, F32_W_TOL, F32_DX_TOL, F32_GRAD_TOL = 1e-3, 1e-3, 1e-3, 2e-2
# production bf16 mode against the emulation: the per-block gates of tests/test_gpu_emulation.py (restated)
BLOCK_Y_TOL, BLOCK_DX_TOL, BLOCK_GRAD_TOL = 2e-3, 8e-3, 1.2e-2


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def lib():
    from pevit_amd import _lib
    return _lib.load()


# ----------------------------------------------------------------------------------------------------------- the kernel
# The lse that the production attention kernels save is m + log(l) with l the sum of the bf16-ROUNDED probabilities (attention.hip:
# the normaliser their P.V product and the backward use).  exp(S - lse) with that lse therefore sums to 1 only within the relative
# rounding of l: |l - sum p| <= 2^-9 sum p, so a row sums to 1 within 1 / (1 - 2^-9) - 1 = 1.96e-3.  The kernel itself is held to
# f32-class accuracy (1e-5 absolute) twice: against softmax with an exact lse, and against exp(S - lse) with the saved lse.
BF16_LSE_ROWSUM_TOL = 2.1e-3


@pytest.mark.parametrize("N", [10, 50, 197, 257])
def test_probs_kernel_matches_softmax(lib, N):
    from pevit_amd import _lib
    B, H = 3, 4
    g = torch.Generator().manual_seed(N)
    q = (torch.randn(B * H, N, 64, generator=g) * 0.4).bfloat16().cuda()
    k = (torch.randn(B * H, N, 64, generator=g) * 0.4).bfloat16().cuda()
    v = torch.randn(B * H, N, 64, generator=g).bfloat16().cuda()
    out = torch.empty(B * N, H * 64, dtype=torch.bfloat16, device="cuda")
    lse_fwd = torch.empty(B * H * N, dtype=torch.float32, device="cuda")
    S = lambda: _lib.stream_ptr()
    P = _lib.ptr
    _lib.check(lib.pevit_op_attn_fwd(S(), P(q), P(k), P(v), P(out), H * 64, P(lse_fwd), B, H, N), "attn_fwd")
    s64 = torch.bmm(q.double(), k.double().transpose(1, 2))
    lse_exact = torch.logsumexp(s64, dim=-1).float().reshape(-1).contiguous()
    torch.cuda.synchronize()
    for lse, rowsum_tol in ((lse_exact, 1e-5), (lse_fwd, BF16_LSE_ROWSUM_TOL)):
        mean = torch.full((B, N, N), float("nan"), device="cuda")
        heads = torch.full((B, H, N, N), float("nan"), device="cuda")
        _lib.check(lib.pevit_op_attn_probs(S(), P(q), P(k), P(lse), P(mean), B, H, N, 1), "attn_probs mean")
        _lib.check(lib.pevit_op_attn_probs(S(), P(q), P(k), P(lse), P(heads), B, H, N, 0), "attn_probs heads")
        torch.cuda.synchronize()
        ref = torch.exp(s64 - lse.double().view(B * H, N, 1)).view(B, H, N, N)
        if lse is lse_exact:
            assert float((ref - torch.softmax(s64, dim=-1).view(B, H, N, N)).abs().max()) < 1e-6
        for got, want in ((heads, ref), (mean, ref.sum(1) / H)):
            got = got.double()
            assert torch.isfinite(got).all()
            assert float((got.sum(-1) - 1).abs().max()) < rowsum_tol
            assert float((got - want).abs().max()) < 1e-5
# ----------------------------------------------------------------------------------------------------------- the seam
def _model(method, weight_format="bf16", seed=4):
    from oracle import ref_cpu
    from pevit_amd.evaluation.model import build_peft_model
    from pevit_amd.synth import randomize_adapters
    model = build_peft_model(dict(load_tiny_sd()), method).cuda()
    model.visual.weight_format = weight_format
    named = [(n, p) for n, p in model.visual.named_parameters() if ref_cpu.is_trainable(method, "visual." + n)]
    model.visual.engine()
    randomize_adapters([(n, p) for n, p in named], seed=seed)
    for _, p in named:
        p.requires_grad_(True)
    return model, named


def _oracle_params(model, method, requires_grad=True):
    from oracle import ref_cpu
    p = {"visual." + k: v.detach().cpu().clone() for k, v in model.visual.state_dict().items()}
    if requires_grad:
        for k in p:
            if ref_cpu.is_trainable(method, k):
                p[k].requires_grad_(True)
    return p


def _oracle_weights(x, p, a, t, heads, method):
    """softmax weights restated from the oracle's pieces (model.py:786-828): q (scaled, + the raw-reshaped delta) and k."""
    from oracle import ref_cpu
    N, B, E = x.shape
    hd = E // heads
    qkv = ref_cpu._linear(x, p[a + "in_proj_weight"], p[a + "in_proj_bias"])
    q, k, _ = qkv.chunk(3, dim=-1)
    q = ref_cpu._heads(q, N, B, heads, hd) / math.sqrt(hd)
    k = ref_cpu._heads(k, N, B, heads, hd)
    if method == "kadaptation":
        q = q.contiguous() + ref_cpu.kadapt_delta(x, p, a, t, "q").reshape(B * heads, N, hd)
    elif method == "lora":
        q = q.contiguous() + ref_cpu.lora_delta(x, p[a + "q_proj_adapter1.weight"], p[a + "q_proj_adapter2.weight"]).reshape(B * heads, N, hd)
    w = torch.softmax(torch.bmm(q, k.transpose(-2, -1)), dim=-1).view(B, heads, N, N)
    return w


def _layer_grads(model, named, p, layer):
    """(engine gradient, oracle gradient) of the trainable tensors a seam call of `layer` touches; the others must be zero"""
    out = {}
    for n, prm in named:
        mine = f"resblocks.{layer}.attn." in n or n.startswith("transformer.phm_rule")
        ge = prm.grad.detach().cpu() if prm.grad is not None else torch.zeros_like(prm.detach().cpu())
        go = p["visual." + n].grad
        if mine and go is not None:
            out[n] = (ge, go)
        else:
            assert float(ge.abs().max()) == 0.0, n
    return out


@pytest.mark.parametrize("method", METHODS)
def test_seam_f32_verify_vs_oracle(method):
    from oracle import ref_cpu
    model, named = _model(method, "f32-verify")
    arch = model.visual.arch
    layer, B = 1, 3
    attn = model.visual.transformer.resblocks[layer].attn
    g = torch.Generator().manual_seed(21)
    x = torch.randn(arch.tokens, B, arch.width, generator=g)
    dy = torch.randn(arch.tokens, B, arch.width, generator=g)
    p = _oracle_params(model, method)
    a, t = f"visual.transformer.resblocks.{layer}.attn.", "visual.transformer."
    xr = x.clone().requires_grad_(True)
    if method in ("kadaptation", "lora"):
        y_ref = ref_cpu.attention_site_mha(xr, p, a, t, arch.heads, method)
    else:
        y_ref = ref_cpu.stock_mha(xr, p, a, arch.heads)
    y_ref.backward(dy)
    with torch.no_grad():
        w_ref = _oracle_weights(x, p, a, t, arch.heads, method)
    xc = x.cuda().requires_grad_(True)
    y, w = attn(xc, xc, xc)
    _, wh = attn(xc, xc, xc, average_attn_weights=False)
    y2, none = attn(xc, xc, xc, need_weights=False)
    assert none is None and w.shape == (B, arch.tokens, arch.tokens) and wh.shape == (B, arch.heads, arch.tokens, arch.tokens)
    for pr in model.visual.parameters():
        pr.grad = None
    y2.backward(dy.cuda())
    torch.cuda.synchronize()
    assert rel_err(y.detach().cpu(), y_ref.detach()) < F32_Y_TOL
    assert torch.equal(y.detach(), y2.detach())
    assert rel_err(w.detach().cpu(), w_ref.sum(1) / arch.heads) < F32_W_TOL
    assert rel_err(wh.detach().cpu(), w_ref) < F32_W_TOL
    assert float((w.detach().sum(-1) - 1).abs().max()) < 1e-5
    assert rel_err(xc.grad.cpu(), xr.grad) < F32_DX_TOL
    grads = _layer_grads(model, named, p, layer)
    if method in ("kadaptation", "lora"):
        assert grads
    for n, (ge, go) in grads.items():
        assert rel_err(ge, go) < F32_GRAD_TOL, n


@pytest.mark.parametrize("method", METHODS)
def test_seam_bf16_vs_emulation(method):
    from oracle import emul_bf16, ref_cpu
    model, named = _model(method)
    arch = model.visual.arch
    layer, B = 0, 5
    attn = model.visual.transformer.resblocks[layer].attn
    g = torch.Generator().manual_seed(22)
    # bf16-valued input and upstream gradient: the engine's first act on both is a bf16 cast, exact here on both sides
    x = torch.randn(arch.tokens, B, arch.width, generator=g).bfloat16().float()
    dy = torch.randn(arch.tokens, B, arch.width, generator=g).bfloat16().float()
    p = _oracle_params(model, method)
    a, t = f"visual.transformer.resblocks.{layer}.attn.", "visual.transformer."
    xr = x.clone().requires_grad_(True)
    wc = emul_bf16.make_wcache(p)
    if method in ("kadaptation", "lora"):
        y_em = emul_bf16.attention_site(xr, p, a, t, arch.heads, method, wc)
    else:
        y_em = emul_bf16.stock_attention(xr, p, a, arch.heads, wc)
    y_em.backward(dy)
    xc = x.cuda().requires_grad_(True)
    for pr in model.visual.parameters():
        pr.grad = None
    y, w = attn(xc, xc, xc)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    assert rel_err(y.detach().cpu(), y_em.detach()) < BLOCK_Y_TOL
    assert rel_err(xc.grad.cpu(), xr.grad) < BLOCK_DX_TOL
    assert float((w.sum(-1) - 1).abs().max()) < BF16_LSE_ROWSUM_TOL and float(w.min()) >= 0
    grads = _layer_grads(model, named, p, layer)
    for n, (ge, go) in grads.items():
        assert rel_err(ge, go) < BLOCK_GRAD_TOL, n


@pytest.mark.parametrize("method", METHODS)
def test_seam_composes_to_the_block(method):
    """f32-verify: x + attn(ln_1(x))[0], then the MLP half of the block from the oracle, equals resblocks[i](x)."""
    from oracle import ref_cpu
    model, _ = _model(method, "f32-verify")
    arch = model.visual.arch
    layer, B = 1, 2
    blk = model.visual.transformer.resblocks[layer]
    x = torch.randn(arch.tokens, B, arch.width, generator=torch.Generator().manual_seed(23)).cuda()
    with torch.no_grad():
        y_blk = blk(x).cpu()
        xn = F.layer_norm(x, (arch.width,), blk.ln_1.weight, blk.ln_1.bias, 1e-5)
        x2 = (x + blk.attn(xn, xn, xn, need_weights=False)[0]).cpu()
        p = _oracle_params(model, method, requires_grad=False)
        pre, t = f"visual.transformer.resblocks.{layer}.", "visual.transformer."
        h = ref_cpu.mlp(ref_cpu.layer_norm(x2, p[pre + "ln_2.weight"], p[pre + "ln_2.bias"]), p, pre)
        if method == "adapter":
            y = x2 + ref_cpu.bottleneck_adapter(h, h, p, pre + "adapter.")
        elif method == "compacter":
            y = x2 + ref_cpu.compacter_adapter(h, p, pre + "compacter.", p[t + "phm_rule"])
        else:
            y = x2 + h
    assert rel_err(y, y_blk) < 1e-4


def test_saved_state_rules():
    from pevit_amd import _lib
    model, _ = _model("kadaptation")
    arch = model.visual.arch
    blk = model.visual.transformer.resblocks[1]
    eng = model.visual.engine()
    x = torch.randn(arch.tokens, 2, arch.width, device="cuda")
    # a block forward through the same layer after the seam's forward: the seam's backward raises
    xs = x.clone().requires_grad_(True)
    y, _ = blk.attn(xs, xs, xs)
    blk(x)
    with pytest.raises(RuntimeError, match="no longer holds"):
        y.sum().backward()
    # ... and the reverse
    xb = x.clone().requires_grad_(True)
    z = blk(xb)
    blk.attn(x, x, x)
    with pytest.raises(RuntimeError, match="no longer holds"):
        z.sum().backward()
    # the C ABI refuses the mismatched backward by itself as well
    eng.attention_forward(x, 1)
    with pytest.raises(_lib.PevitError, match="attention_forward"):
        eng.blocks_backward(x, 1, 2)
    eng.attention_forward(x, 1)
    with pytest.raises(_lib.PevitError, match="layer 0"):
        eng.attention_backward(x, 0)
    eng.blocks_forward(x, 1, 2)
    with pytest.raises(_lib.PevitError, match="transformer_forward"):
        eng.attention_backward(x, 1)
    # a gradient through the weights
    xw = x.clone().requires_grad_(True)
    _, w = blk.attn(xw, xw, xw)
    with pytest.raises(RuntimeError, match="no gradient through attention weights"):
        w.sum().backward()


def test_fp8_act_is_refused():
    from pevit_amd import _lib
    from pevit_amd.engine import HipEngine, adapter_param_spec
    from pevit_amd.synth import ARCHS, synth_state_dict
    arch = ARCHS["tiny-128"]
    sd = {k: v for k, v in synth_state_dict(arch, seed=2, text_tower=False).items() if k.startswith("visual.")}
    sd.update({n: torch.zeros(s) for n, s, _ in adapter_param_spec("kadaptation", arch.width, arch.layers)})
    e = HipEngine(arch, "kadaptation", 10, 2, weight_format="fp8-act")
    e.load_state_dict(sd)
    with pytest.raises(_lib.PevitError, match="fp8-act"):
        e.attention_forward(torch.zeros(arch.tokens, 2, arch.width, device="cuda"), 0)


@pytest.mark.parametrize("arch_name,method,B", [("tiny-128", "kadaptation", 6), ("tiny-256", "lora", 5), ("tiny-n257", "kadaptation", 4),
                                                 ("tiny-256", "none", 4)])
def test_fp8_seam_is_bit_identical_to_bf16_on_dequantised_weights(arch_name, method, B):
    from test_gpu_fp8 import _engines
    arch, e8, e16, _, _, _ = _engines(arch_name, method, B)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(arch.tokens, B, arch.width, generator=g).cuda()
    dy = torch.randn(arch.tokens, B, arch.width, generator=g).cuda()
    for layer in range(arch.layers):
        y8, w8 = e8.attention_forward(x, layer, weights="heads")
        y16, w16 = e16.attention_forward(x, layer, weights="heads")
        e8.zero_grad(); e16.zero_grad()
        dx8, dx16 = e8.attention_backward(dy, layer), e16.attention_backward(dy, layer)
        torch.cuda.synchronize()
        assert torch.equal(y8, y16) and torch.equal(w8, w16) and torch.equal(dx8, dx16), layer
        assert torch.equal(e8.grads, e16.grads), layer
        if method != "none":
            assert float(e8.grads.abs().max()) > 0
