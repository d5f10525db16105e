"""Host side of tests/test_gpu_adapter_fused.py (no GPU): the inputs of the per-launch tests of adapter_fwd_kernel / adapter_bwd_kernel
(csrc/adapter_fused.hip), their float64 references, the assertions themselves, and the evidence that those assertions can see what
they are meant to see.

The kernels take 32 token rows per workgroup through  h = hraw + bpr -> LayerNorm -> z (bf16) -> z Wd^T + b_down -> activation
(bf16; gelu_new also keeps its bf16 pre-activation) -> act Wu^T -> x_out = x_mid + h + up + b_up,  and backwards through
d pre = (dy Wu) act'(saved) (bf16) -> d z = d pre Wd -> LayerNorm backward with the column sums of dz * xhat, dz and dx_out per
workgroup -> dh = bf16(dx_out + LN'(dz)).  This file states, on the CPU and with the kernels nowhere in sight:

  * the input recipe (`case`): a large c_proj bias (0.5 sigma) so that an x-hat formed without it shows;
  * the float64 references on h = f32(hraw + bpr) widened, the operand the kernels form:
      staged -- every stage from the STORED operands of the stage before it (`check_forward` / `check_backward` take the outputs of
                one launch and recompute each stage from what that launch stored, so one rounding flip cannot leak downstream);
                the column sums per workgroup block, over exactly that block's valid rows;
      pure   -- no intermediate rounding at all (`forward64(..., q=None)`);
  * `bf16_close`, the comparison of every bf16 output: with r = bf16(ref64) rounded to nearest even, an element may differ from r
    only if |got - ref64| <= one bf16 ulp at r or <= 2^-18 max|ref64| (cancellation around z ~ 0 and pre ~ 0, ReLU sign flips at
    pre ~ 0), and at most 1 % of the elements may differ at all.  The cap is a condition, not a measurement: the same forward and
    backward in torch float32 arithmetic differ from the float64 staged reference on < 0.1 % of the elements for every (E, act) --
    `test_float32_proxy_stays_far_inside_the_cap` runs the very same assertions with the cap at 1e-3 (worst share here: 2.3e-4);
  * the rounding floor (`floors`): float64 arithmetic with the kernels' bf16 rounding points against the pure reference, per case:
    x_out 7e-4 .. 1.2e-3 and act 2.8e-3 .. 5.2e-3 max-rel at T = 70.  The GPU file holds the kernels' end-to-end error to
    FLOOR_FACTOR = 2 of it (ties that round differently under f32 and f64 accumulation moved < 3e-4 of the elements here);
  * the bite: seven wrong kernels, each as a mutant of the float64 emulation, each of which must FAIL those assertions at every E:
      (a) x-hat of the backward from hraw without bpr                  (b) the last valid row counted twice in the column sums
      (c) all 31 pad rows of the second tile counted at T = 33         (d) gelu_new' evaluated on act instead of apre
      (e) the last 16 of the E columns dropped from the down product   (f) bf16 truncation instead of round-to-nearest
      (g) the residual and the d b_up sums from the wrong one of dres / dyb
    (a) moves dh by 6e-3 .. 1e-2 of its largest magnitude only, and (g) by half a bf16 ulp: they are why dh is held to bf16_close.

The emulation is the reference here, never the kernel.  `pytest -s` prints the floors and the proxy's shares.
"""
import functools
import math

import pytest
import torch

from conftest import max_rel

ROWS = 32                                   # token rows per workgroup of the fused kernels (== pevit_op_adapter_blocks' divisor)
GRID_E = (256, 512, 768, 1024)              # NV = E / 256 = 1..4
ACTS = (0, 1)                               # 0 = ReLU (Adapter), 1 = gelu_new (Compacter)
GRID_T = (1, 33, 64, 70)                    # a single row; a one-row second tile; exact tiles; a 6-row last tile
BIG_T = 32 * 257 + 5                        # more workgroups than CUs at one workgroup per CU
F32_GATE = 2e-5                             # tests/test_gpu_ops.py test_layernorm_fwd_bwd, f32 outputs
COLSUM_GATE = 1e-4                          # tests/test_gpu_ops2.py test_ln_bwd_affine, column sums
CAP, PROXY_CAP = 1e-2, 1e-3                 # share of bf16 elements that may differ from bf16(ref64): the kernels / the f32 proxy
ABS_BOUND = 2.0 ** -18                      # x max|ref64|: the near-zero bound of bf16_close
FLOOR_FACTOR = 2.0
BF16_KEYS = ("z", "act", "apre", "dpre", "dh")
BF = torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def case(E, T):
    """the operands of one launch pair on the CPU (f32 / bf16), seeded by the shape; never modified"""
    g = torch.Generator(device="cpu").manual_seed(E + T)

    def R(*s, sc=1.0):
        return torch.randn(*s, generator=g) * sc
    c = dict(E=E, T=T)
    c["hraw"] = R(T, E, sc=2.0) + 0.5
    c["bpr"] = R(E, sc=0.5)                 # large on purpose: a dropped bias shows
    c["x_mid"] = R(T, E)
    c["gamma"] = 1 + R(E, sc=0.2)
    c["beta"] = R(E, sc=0.2)
    c["wd"] = R(64, E, sc=E ** -0.5).to(BF)
    c["b_down"] = R(64, sc=0.1)
    c["wu"] = R(E, 64, sc=0.125).to(BF)
    c["b_up"] = R(E, sc=0.1)
    c["dres"] = R(T, E)
    c["dyb"] = c["dres"].to(BF)
    c["wuT"] = c["wu"].t().contiguous()
    c["wdT"] = c["wd"].t().contiguous()
    return c


def on(c, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in c.items()}


# ---------------------------------------------------------------------------------------------------------------- rounding
def bf16_rne(x64):
    """float64 -> bf16, round to nearest even in ONE step (through float32 it would be rounded twice), returned widened"""
    i = x64.contiguous().view(torch.int64)
    i = (i + ((1 << 44) - 1) + ((i >> 45) & 1)) & ~((1 << 45) - 1)
    return i.view(torch.float64)


def bf16_trunc(x64):
    return (x64.contiguous().view(torch.int64) & ~((1 << 45) - 1)).view(torch.float64)


def bf16_ulp(r64):
    """spacing of the bf16 grid at the (bf16-valued) r; 0 at r == 0"""
    _, ex = torch.frexp(r64)
    return torch.where(r64 == 0, torch.zeros_like(r64), torch.ldexp(torch.ones_like(r64), ex - 8))


def bf16_close(got, ref64, cap=CAP, what=""):
    """asserts the rule of the module docstring; returns the share of elements that differ from bf16(ref64)"""
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    g = got.double()
    assert torch.isfinite(g).all(), f"{what}: non-finite element"
    r = bf16_rne(ref64)
    differ = g != r
    err = (g - ref64).abs()
    bad = differ & (err > bf16_ulp(r)) & (err > ABS_BOUND * float(ref64.abs().max()))
    share = float(differ.double().mean())
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements off by more than a bf16 ulp, worst {float(err[bad].max()):.3e}"
    assert share <= cap, f"{what}: {share:.3e} of the elements differ from bf16(ref64), cap {cap:.0e}"
    return share


# ---------------------------------------------------------------------------------------------------------------- float64 stages
K0 = math.sqrt(2.0 / math.pi)


def gelu_new64(x):                          # gemm_epilogue.h gelu_new_f
    return 0.5 * x * (1 + torch.tanh(K0 * (x + 0.044715 * x ** 3)))


def gelu_new_grad64(x):                     # gemm_epilogue.h gelu_new_grad_f
    t = torch.tanh(K0 * (x + 0.044715 * x ** 3))
    return 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * K0 * (1 + 3 * 0.044715 * x * x)


def h64(c):
    return (c["hraw"] + c["bpr"]).double()  # f32(hraw + bpr), widened


def ln_stats64(h):
    mean = h.mean(1, keepdim=True)
    return mean, (h.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()


def stage_z(c, h, mean, rstd):
    return (h - mean) * rstd * c["gamma"].double() + c["beta"].double()


def stage_pre(c, z, drop=0):
    """z Wd^T + b_down from a given z; drop: mutant (e), the last `drop` of the E columns left out of the product"""
    k = c["E"] - drop
    return z.double()[:, :k] @ c["wd"].double()[:, :k].t() + c["b_down"].double()


def stage_xout(c, h, act):
    return c["x_mid"].double() + h + (act.double() @ c["wu"].double().t() + c["b_up"].double())


def stage_dpre(c, act_kind, saved):
    s = saved.double()
    return (c["dyb"].double() @ c["wuT"].double().t()) * ((s > 0).double() if act_kind == 0 else gelu_new_grad64(s))


def block_sums(x, T):
    """[T][E] -> [blocks][E]: sums over the rows of each 32-row workgroup block"""
    nb = -(-T // ROWS)
    pad = torch.zeros((nb * ROWS, x.shape[1]), dtype=x.dtype, device=x.device)
    pad[:T] = x
    return pad.view(nb, ROWS, -1).sum(1)


def stage_ln_bwd(c, dpre, mean_a, rstd_a, res, no_bias=False, row_weight=None):
    """d z = d pre Wd, LayerNorm backward, dh and partial[block][3][E] from a given d pre, the given statistics and residual.
    no_bias: mutant (a); row_weight [T]: how often a row enters the column sums (mutants (b), (c))"""
    dz = dpre.double() @ c["wdT"].double().t()
    h = c["hraw"].double() if no_bias else h64(c)
    mean, rstd = mean_a.double().view(-1, 1), rstd_a.double().view(-1, 1)
    xh = (h - mean) * rstd
    gd = dz * c["gamma"].double()
    m1, m2 = gd.mean(1, keepdim=True), (gd * xh).mean(1, keepdim=True)
    r = res.double()
    dh = rstd * (gd - m1 - xh * m2) + r
    w = torch.ones((c["T"], 1), dtype=torch.float64, device=dz.device) if row_weight is None else row_weight.double().view(-1, 1)
    partial = torch.stack([block_sums(w * dz * xh, c["T"]), block_sums(w * dz, c["T"]), block_sums(w * r, c["T"])], dim=1)
    return dh, partial


# ---------------------------------------------------------------------------------------------------------------- whole passes
def forward64(c, act_kind, q=bf16_rne, drop=0):
    """the forward in float64 arithmetic; q: what a bf16 store does (bf16_rne: the emulation; None: the pure reference)"""
    q = q or (lambda x: x)
    h = h64(c)
    mean, rstd = ln_stats64(h)
    z = q(stage_z(c, h, mean, rstd))
    pre = stage_pre(c, z, drop)
    if act_kind == 0:
        apre, act = None, q(pre.clamp(min=0))
    else:
        apre = q(pre)
        act = q(gelu_new64(apre))
    out = dict(z=z, mean_a=mean.view(-1), rstd_a=rstd.view(-1), act=act, x_out=stage_xout(c, h, act))
    if apre is not None:
        out["apre"] = apre
    return out


def backward64(c, act_kind, saved, mean_a, rstd_a, res, q=bf16_rne, **mutant):
    q = q or (lambda x: x)
    dpre = q(stage_dpre(c, act_kind, saved))
    dh, partial = stage_ln_bwd(c, dpre, mean_a, rstd_a, res, **mutant)
    return dict(dpre=dpre, dh=q(dh), partial=partial)


def stored(d):
    """float64 results in the types the kernels store them in"""
    return {k: v.to(BF if k in BF16_KEYS else torch.float32) for k, v in d.items()}


def backward_operands(c, act_kind):
    """saved (act / apre), mean_a, rstd_a of the backward: from the float64 forward of this file, not from the forward kernel"""
    f = stored(forward64(c, act_kind))
    return f["act" if act_kind == 0 else "apre"], f["mean_a"], f["rstd_a"]


def floors(c, act_kind):
    """the rounding floor of the end-to-end comparison: emulation against the pure reference, max-rel.  Also returns the pure
    reference, which is what the kernel's outputs are then held against."""
    e, p = forward64(c, act_kind), forward64(c, act_kind, q=None)
    return {k: max_rel(e[k], p[k]) for k in ("x_out", "act")}, p


# ---------------------------------------------------------------------------------------------------------------- the assertions
def check_forward(got, c, act_kind, cap=CAP):
    """the staged assertions on the outputs of ONE forward launch (payloads [T][..]); returns the measured figures"""
    h = h64(c)
    mean, rstd = ln_stats64(h)
    fig = dict(mean=max_rel(got["mean_a"], mean.view(-1)), rstd=max_rel(got["rstd_a"], rstd.view(-1)))
    assert fig["mean"] < F32_GATE and fig["rstd"] < F32_GATE, fig
    fig["z"] = bf16_close(got["z"], stage_z(c, h, mean, rstd), cap, "z")
    pre = stage_pre(c, got["z"])                                   # from the launch's own stored z
    if act_kind == 0:
        fig["act"] = bf16_close(got["act"], pre.clamp(min=0), cap, "act")
    else:
        fig["apre"] = bf16_close(got["apre"], pre, cap, "apre")
        fig["act"] = bf16_close(got["act"], gelu_new64(got["apre"].double()), cap, "act")      # from its own stored apre
    fig["x_out"] = max_rel(got["x_out"], stage_xout(c, h, got["act"]))                          # from its own stored act
    assert fig["x_out"] < F32_GATE, fig
    return fig


def check_backward(got, c, act_kind, saved, mean_a, rstd_a, res, cap=CAP):
    """the staged assertions on the outputs of ONE backward launch; res: the tensor the residual and the d b_up sums must come
    from (dres where it is given, dyb where it is not)"""
    fig = dict(dpre=bf16_close(got["dpre"], stage_dpre(c, act_kind, saved), cap, "dpre"))
    dh, partial = stage_ln_bwd(c, got["dpre"], mean_a, rstd_a, res)                             # from its own stored d pre
    fig["dh"] = bf16_close(got["dh"], dh, cap, "dh")
    assert got["partial"].shape == partial.shape, (got["partial"].shape, partial.shape)
    p = got["partial"].double()
    assert torch.isfinite(p).all()
    rel = (p - partial).abs().amax(-1) / (partial.abs().amax(-1) + 1e-30)                       # [block][3]: block by block
    fig["partial"] = float(rel.max())
    assert fig["partial"] < COLSUM_GATE, (fig, rel.argmax().item())
    return fig


# ---------------------------------------------------------------------------------------------------------------- tests
def test_bf16_rounding_helpers():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8 + 2.0 ** -30), 0.0,
                      1.99999, 3.0e-5], dtype=torch.float64)
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6, -(1.0 + 2.0 ** -7), 0.0, 2.0, 0.0], dtype=torch.float64)
    want[-1] = float(torch.tensor(3.0e-5).to(BF))
    assert torch.equal(bf16_rne(x), want)
    # (1 + 2^-8 + 2^-30 rounds to 1 + 2^-8 in float32, a tie that round-to-even would then take DOWN: the reason for the one-step rounding)
    assert float(x[2].float().to(BF)) == 1.0
    r = torch.randn(4096, generator=torch.Generator().manual_seed(0)).double()
    assert torch.equal(bf16_rne(r.float().double()), r.float().to(BF).double())
    assert torch.equal(bf16_ulp(torch.tensor([1.0, 1.5, -2.0, 0.0, 0.75], dtype=torch.float64)),
                       torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 0.0, 2.0 ** -8], dtype=torch.float64))
    assert torch.equal(bf16_trunc(torch.tensor([1.0 + 3 * 2.0 ** -8], dtype=torch.float64)), torch.tensor([1.0 + 2.0 ** -7], dtype=torch.float64))


def test_bf16_close_rule():
    ref = torch.linspace(-4, 4, 4001, dtype=torch.float64)
    r = bf16_rne(ref)
    assert bf16_close(r.to(BF), ref) == 0.0
    up = r.clone()
    up[:30] = r[:30] + bf16_ulp(r[:30]) * torch.where(r[:30] < ref[:30], 1.0, -1.0)      # the neighbour on the other side of ref
    assert 0 < bf16_close(up.to(BF), ref) <= CAP
    with pytest.raises(AssertionError, match="cap"):
        up[:60] = r[:60] + bf16_ulp(r[:60]) * torch.where(r[:60] < ref[:60], 1.0, -1.0)
        bf16_close(up.to(BF), ref)
    two = r.clone()
    two[7] = r[7] + 2 * bf16_ulp(r[7])
    with pytest.raises(AssertionError, match="more than a bf16 ulp"):
        bf16_close(two.to(BF), ref)
    tiny = torch.tensor([4.0, 0.0], dtype=torch.float64)                                   # a sign flip at pre ~ 0 under ReLU
    assert bf16_close(torch.tensor([4.0, 1.0e-5]).to(BF), tiny, cap=1.0) == 0.5
    with pytest.raises(AssertionError, match="more than a bf16 ulp"):
        bf16_close(torch.tensor([4.0, 1.0e-4]).to(BF), tiny, cap=1.0)


def proxy32_forward(c, act_kind):
    """the forward in torch float32 arithmetic with the kernels' stores: stands in for a correct kernel"""
    h = c["hraw"] + c["bpr"]
    mean = h.mean(1, keepdim=True)
    rstd = (h.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    z = ((h - mean) * rstd * c["gamma"] + c["beta"]).to(BF)
    pre = z.float() @ c["wd"].float().t() + c["b_down"]
    out = dict(z=z, mean_a=mean.view(-1), rstd_a=rstd.view(-1))
    if act_kind == 0:
        out["act"] = pre.clamp(min=0).to(BF)
    else:
        out["apre"] = pre.to(BF)
        out["act"] = gelu_new64(out["apre"].float()).to(BF)
    out["x_out"] = (c["x_mid"] + h) + (out["act"].float() @ c["wu"].float().t() + c["b_up"])
    return out


def proxy32_backward(c, act_kind, saved, mean_a, rstd_a, res):
    s = saved.float()
    dpre = ((c["dyb"].float() @ c["wuT"].float().t()) * ((s > 0).float() if act_kind == 0 else gelu_new_grad64(s))).to(BF)
    dz = dpre.float() @ c["wdT"].float().t()
    xh = ((c["hraw"] + c["bpr"]) - mean_a.view(-1, 1)) * rstd_a.view(-1, 1)
    gd = dz * c["gamma"]
    m1, m2 = gd.mean(1, keepdim=True), (gd * xh).mean(1, keepdim=True)
    r = res.float()
    dh = (rstd_a.view(-1, 1) * (gd - m1 - xh * m2) + r).to(BF)
    T = c["T"]
    return dict(dpre=dpre, dh=dh, partial=torch.stack([block_sums(dz * xh, T), block_sums(dz, T), block_sums(r, T)], dim=1))


@pytest.mark.parametrize("act_kind", ACTS)
@pytest.mark.parametrize("E", GRID_E)
def test_float32_proxy_stays_far_inside_the_cap(E, act_kind):
    """the 1 % cap and the 2^-18 bound are conditions a correct kernel meets with room: float32 arithmetic, held to the very
    assertions of the GPU file with the cap at 0.1 %"""
    c = case(E, 70)
    fig = check_forward(proxy32_forward(c, act_kind), c, act_kind, cap=PROXY_CAP)
    saved, mean_a, rstd_a = backward_operands(c, act_kind)
    for name, res in (("dres", c["dres"]), ("dyb", c["dyb"])):
        b = check_backward(proxy32_backward(c, act_kind, saved, mean_a, rstd_a, res), c, act_kind, saved, mean_a, rstd_a, res,
                           cap=PROXY_CAP)
        fig.update({f"{k}[{name}]": v for k, v in b.items()})
    print(f"\nE={E} act={act_kind} f32 proxy: " + "  ".join(f"{k} {v:.1e}" for k, v in fig.items()), end="")


@pytest.mark.parametrize("act_kind", ACTS)
@pytest.mark.parametrize("E", GRID_E)
def test_rounding_floor_and_emulation_passes_its_own_assertions(E, act_kind):
    """the emulation passes every staged assertion with nothing differing; its distance to the pure reference is the floor"""
    for T in GRID_T:
        c = case(E, T)
        fig = check_forward(stored(forward64(c, act_kind)), c, act_kind, cap=0.0)
        saved, mean_a, rstd_a = backward_operands(c, act_kind)
        for res in (c["dres"], c["dyb"]):
            check_backward(stored(backward64(c, act_kind, saved, mean_a, rstd_a, res)), c, act_kind, saved, mean_a, rstd_a, res, cap=0.0)
        fl, _ = floors(c, act_kind)
        print(f"\nE={E} act={act_kind} T={T}: floor x_out {fl['x_out']:.2e}  act {fl['act']:.2e}", end="")
        assert 1e-4 < fl["x_out"] < 5e-3 and 5e-4 < fl["act"] < 1.6e-2, fl      # bf16 rounding of act: 2^-9 relative at the most per element


def _fails(fn, *a, **k):
    try:
        fn(*a, **k)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("E", GRID_E)
def test_the_staged_assertions_bite(E):
    """each wrong kernel of the module docstring, as a mutant of the float64 emulation, fails the assertions of the GPU file"""
    for act_kind in ACTS:
        c = case(E, 70)
        saved, mean_a, rstd_a = backward_operands(c, act_kind)
        args = (c, act_kind, saved, mean_a, rstd_a)

        def bwd_fails(res_used, res_expected, a=args, **mutant):
            return _fails(check_backward, stored(backward64(*a, res_used, **mutant)), *a, res_expected)
        for res in (c["dres"], c["dyb"]):
            assert not bwd_fails(res, res)                                                         # the unmutated emulation passes
            assert bwd_fails(res, res, no_bias=True), "(a)"
            twice = torch.ones(70)
            twice[-1] = 2
            assert bwd_fails(res, res, row_weight=twice), "(b)"
            assert bwd_fails(res, res, q=bf16_trunc), "(f) backward"
        assert bwd_fails(c["dyb"], c["dres"]), "(g) dres given, dyb used"
        assert bwd_fails(c["dres"], c["dyb"]), "(g) dres absent, an f32 copy used"
        if act_kind == 1:
            act = stored(forward64(c, 1))["act"]
            assert _fails(check_backward, stored(backward64(c, 1, act, mean_a, rstd_a, c["dres"])), *args, c["dres"]), "(d)"
        assert not _fails(check_forward, stored(forward64(c, act_kind)), c, act_kind)
        assert _fails(check_forward, stored(forward64(c, act_kind, drop=16)), c, act_kind), "(e)"
        assert _fails(check_forward, stored(forward64(c, act_kind, q=bf16_trunc)), c, act_kind), "(f) forward"
        # (c) at T = 33: the second tile's one valid row counted for all 32
        c33 = case(E, 33)
        a33 = (c33, act_kind) + backward_operands(c33, act_kind)
        pads = torch.ones(33)
        pads[-1] = 32
        assert not _fails(check_backward, stored(backward64(*a33, c33["dres"])), *a33, c33["dres"])
        assert _fails(check_backward, stored(backward64(*a33, c33["dres"], row_weight=pads)), *a33, c33["dres"]), "(c)"


@pytest.mark.parametrize("struct,cls", [("pevit_adapter_fwd_args", "PevitAdapterFwdArgs"), ("pevit_adapter_bwd_args", "PevitAdapterBwdArgs")])
def test_argument_structs_mirror_the_header(struct, cls):
    """the ctypes structures of the two test-only entry points name the header's members in the header's order, pointers as
    pointers and the rest int32"""
    import ctypes
    import os
    import re
    from conftest import ROOT
    from pevit_amd import _lib
    src = open(os.path.join(ROOT, "include", "pevit_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
    members = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        if decl.startswith("int32_t"):
            members += [(n.strip(), ctypes.c_int32) for n in decl[len("int32_t"):].split(",")]
        else:
            assert "*" in decl, decl
            members.append((decl.split("*")[-1].strip(), ctypes.c_void_p))
    assert getattr(_lib, cls)._fields_ == members
