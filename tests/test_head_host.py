"""Host side of tests/test_gpu_head.py (no GPU): the inputs of the per-launch tests of the classifier head (csrc/stem_head.hip:
bn_fwd_kernel, small_gemm_kernel x 3, ce_loss_kernel, ce_kernel + loss_mean_kernel, bce_loss_kernel, bn_bwd_kernel, all behind
pevit_launch_head and reached one launch sequence at a time through the test-only pevit_op_head_ex), their float64 references, the
assertions (`check_head`, `check_identity`), the rounding floors the forward gates are taken from and the evidence that the assertions
can see what they are meant to see.  No kernel runs here: the emulation is the reference, never the kernel.

  * inputs (`case`, seeded by the shape, never modified): feat ~ 1.5 N(0,1) + 0.3 with the LAST ROW DOUBLED, W and bias ~ 0.2 N(0,1)
    with the last class and the last feature column doubled (a dropped batch row or K tail moves whole outputs), running statistics
    away from (0, 1), gW / gb starting from non-zero values (0.05 N(0,1): accumulate and overwrite differ), labels that hold the
    classes 0, 63, 64 and C - 1 wherever C allows.  Variants: "plain"; "ignore" (rows 0, B - 1 and every row b % 7 == 3 carry
    ignore_index -100; at B = 2 only row 0, or no valid row would be left and torch's own answer is NaN); "bad" (row 1 holds the label
    C, row B - 1 the label -1: the two values next to the valid range, so that even a wrong kernel stays inside the allocation);
    "multihot" / "soft" (BCE targets).
  * references (`head_ref`): F.batch_norm(momentum 0.1, eps 1e-5, no affine) -> F.linear -> F.cross_entropy or
    F.binary_cross_entropy_with_logits with torch.autograd on the f32 inputs, in float64 (the reference) and in float32 (torch's own
    distance from float64, printed next to every GPU figure).  Out-of-range labels: torch refuses them; the documented result of the
    kernels is NaN in that row's dlogits and row loss, in the loss and in everything that sums over the batch (gW, gb, and the
    training-mode dfeat), with every other row right -- `head_ref` computes those other rows with the bad labels replaced by class 0
    (a row's dlogits depend on its own label and on the number of non-ignored rows only) and `nan_masks` states where NaN must sit.
  * emulation (`head32`): the kernels' arithmetic in torch float32.  Batch statistics in bn_fwd_kernel's order (16 row groups, each
    summed in row order, then the 16 partials in order); the logits one product at a time in f32 (K roundings per element: the upper
    model tests/test_lowrank_host.py uses for a matrix-core accumulator); rsqrtf perturbed by -1, 0, +1 ulp (the HIP math API states
    1 ulp for it) with the largest floor taken; no fused multiply-add (the device code contracts: fewer roundings, not more).
    Floors = emulation against float64, max-rel; gate = min(cap, 2 x max(floor, 2^-24)) with the caps 1e-5 (ybn, rstd, logits: the
    logits gate of test_head_batchnorm_linear_cross_entropy) and 1e-6 (running statistics).  The factor 2 is the house factor of
    tests/test_lowrank_host.py, for the reason given there.  Measured here (`pytest -s` prints them per case):
        ybn 1.1e-7 .. 2.1e-7   rstd 9.6e-8 .. 2.2e-7   running mean 4.0e-8 .. 8.8e-8   running var 3.7e-8 .. 1.1e-7   logits 1.0e-7 .. 1.2e-6
    Everything behind the loss goes through the hardware's exp / log / reciprocal approximations, which no CPU emulation models; it
    keeps the project's gates: 2e-5 max-rel for dlogits, gW, gb, dybn, dfeat and 1e-5 absolute for the loss and for every row loss.
    (The one-product-at-a-time model is an upper model made for the forward floors only: at D >= 512, where logits reach 25 and more,
    its row losses are 1.3e-5 .. 3.8e-5 from float64, and torch's own float32 row losses 7.3e-6 .. 2.3e-5.  The emulation that must
    pass every assertion, and that the mutants are made from, rounds each product sum once: its row losses stay below the 1e-5 gate at every shape.)
    dfeat_bf16 is exact: the bits of the round-to-nearest-even bf16 of the f32 dfeat that the same launch wrote.
  * the bite (test_every_mutant_fails_wherever_it_differs): each wrong head below, as a mutant of `head32`, must FAIL `check_head`
    (or `check_identity`) at every case, mode and variant at which its outputs differ from the right emulation's in any bit; the right
    emulation must pass everywhere; every mutant differs somewhere.
      (a) running variance from the biased variance      (b) running statistics updated in eval mode
      (c) the last batch row left out of the batch statistics
      (d) the K tail behind the last whole 8-k chunk dropped: d_logits (K = D), d_gw (K = B, gb's row sums included), d_dybn (K = C)
      (e) gW overwritten                                   (f) gb overwritten (f_over); gb added once per 32-column tile (f_tiles)
      (g) the cross-entropy mean over B                    (h) an ignored row keeping its dlogits row
      (i) columns >= 64 (i64) / >= 128 (i128) missing from the softmax sum
      (j) the label's logit taken from the other 64-column half
      (k) rows >= 128 computed from row B - 1              (l) training backward without yhat * mean(dy * yhat)
      (m) eval backward with the means subtracted          (n) dfeat_bf16 truncated
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import max_rel
from test_lowrank_host import FLOOR_FACTOR, ULP

GRID = [(2, 16, 1), (7, 20, 3), (5, 6, 10), (17, 72, 63), (16, 64, 64), (33, 64, 65), (128, 64, 127), (129, 64, 128), (129, 64, 129),
        (257, 64, 100), (128, 512, 1000), (64, 768, 397), (2048, 64, 3), (2049, 64, 3), (2049, 64, 130)]      # (B, D, C)
BCE_GRID = [(7, 20, 3), (129, 64, 129), (64, 768, 397)]
BAD_GRID = [(7, 20, 3), (33, 64, 65), (129, 64, 129)]
OFFSET_GRID = [(7, 20, 3), (129, 64, 128)]
FORM_GRID = [(7, 20, 3), (129, 64, 129), (2049, 64, 3)]
IDENTITY_C = (3, 130)
IGNORE = -100
LOGITS_GATE, RUNNING_GATE, GRAD_GATE, LOSS_GATE = 1e-5, 1e-6, 2e-5, 1e-5      # test_head_batchnorm_linear_cross_entropy's gates
FWD_KEYS = ("ybn", "rstd", "rm", "rv", "logits")
FWD_CAPS = dict(ybn=LOGITS_GATE, rstd=LOGITS_GATE, logits=LOGITS_GATE, rm=RUNNING_GATE, rv=RUNNING_GATE)
GRAD_KEYS = ("dlogits", "gW", "gb", "dybn", "dfeat")
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
MUTANTS = ("a", "b", "c", "d_logits", "d_gw", "d_dybn", "e", "f_over", "f_tiles", "g", "h", "i64", "i128", "j", "k", "l", "m", "n")


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


# ---------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def case(B, D, C, variant="plain"):
    g = torch.Generator(device="cpu").manual_seed(1000003 * B + 1009 * D + C)

    def R(*s, sc=1.0):
        return torch.randn(*s, generator=g) * sc
    c = dict(B=B, D=D, C=C, variant=variant)
    c["feat"] = R(B, D, sc=1.5) + 0.3
    c["feat"][-1] *= 2
    c["W"] = R(C, D, sc=0.2)
    c["W"][-1] *= 2
    c["W"][:, -1] *= 2
    c["bias"] = R(C, sc=0.2)
    c["rm0"] = R(D, sc=0.1)
    c["rv0"] = R(D, sc=0.1).abs() + 0.5
    c["gW0"] = R(C, D, sc=0.05)
    c["gb0"] = R(C, sc=0.05)
    labels = torch.randint(0, C, (B,), generator=g)
    multihot = (torch.rand(B, C, generator=g) < 0.3).float()
    soft = torch.rand(B, C, generator=g)
    c["labels"], c["targets"] = None, None
    if variant in ("multihot", "soft"):
        c["targets"] = multihot if variant == "multihot" else soft
        return c
    ignored = set()
    if variant == "ignore":
        ignored = {0} if B == 2 else {0, B - 1} | {b for b in range(B) if b % 7 == 3}
    bad = {}
    if variant == "bad":
        bad = {1: C, B - 1: -1}
    free = [b for b in range(B) if b not in ignored and b not in bad]
    forced = [k for k in dict.fromkeys((0, 63, 64, C - 1)) if k < C]
    for i, k in enumerate(forced):               # from the back as well, so that rows >= 128 hold both halves where B allows
        if i < len(free):
            labels[free[i]] = k
        if len(free) - 1 - i >= len(forced):
            labels[free[len(free) - 1 - i]] = k
    for b in ignored:
        labels[b] = IGNORE
    for b, v in bad.items():
        labels[b] = v
    c["labels"] = labels
    return c


def bad_rows(c):
    lab = c["labels"]
    if lab is None:
        return torch.zeros(c["B"], dtype=torch.bool)
    return (lab != IGNORE) & ((lab < 0) | (lab >= c["C"]))


@functools.lru_cache(maxsize=None)
def identity_pair(C):
    """(2049, 64, C) with row 2048 ignored, and its first 2048 rows as a case of their own: the one-workgroup cross entropy and the
    ce_kernel + loss_mean_kernel pair then divide by the same 2048 valid rows, and the ignored row adds +0.0 last in lane 0"""
    big = dict(case(2049, 64, C))
    big["labels"] = big["labels"].clone()
    big["labels"][2048] = IGNORE
    big["variant"] = "tail-ignored"
    small = dict(big, B=2048, feat=big["feat"][:2048].clone(), labels=big["labels"][:2048].clone(), variant="first-2048")
    return big, small


# ---------------------------------------------------------------------------------------------------------------- references
_REF = {}


def head_ref(c, training, dtype=F64):
    key = (c["B"], c["D"], c["C"], c["variant"], bool(training), dtype)
    if key in _REF:
        return _REF[key]
    f = c["feat"].detach().to(dtype).clone().requires_grad_(True)
    W = c["W"].detach().to(dtype).clone().requires_grad_(True)
    b = c["bias"].detach().to(dtype).clone().requires_grad_(True)
    rm, rv = c["rm0"].to(dtype).clone(), c["rv0"].to(dtype).clone()
    ybn = F.batch_norm(f, rm, rv, None, None, bool(training), 0.1, 1e-5)
    ybn.retain_grad()
    logits = F.linear(ybn, W, b)
    logits.retain_grad()
    o = {}
    if c["targets"] is not None:
        loss = F.binary_cross_entropy_with_logits(logits, c["targets"].to(dtype))
    else:
        lab = torch.where(bad_rows(c), torch.zeros_like(c["labels"]), c["labels"])
        loss = F.cross_entropy(logits, lab)
        o["rowloss"] = F.cross_entropy(logits.detach(), lab, reduction="none")
    loss.backward()
    var = f.detach().var(0, unbiased=False) if training else c["rv0"].to(dtype)
    o.update(ybn=ybn.detach(), rstd=1.0 / torch.sqrt(var + 1e-5), rm=rm, rv=rv, logits=logits.detach(), loss=loss.detach(),
             dlogits=logits.grad, dybn=ybn.grad, gW=c["gW0"].to(dtype) + W.grad, gb=c["gb0"].to(dtype) + b.grad, dfeat=f.grad)
    _REF[key] = o
    return o


def nan_masks(c, training):
    """where the documented result of out-of-range labels is NaN (all False without such labels)"""
    B, D, C = c["B"], c["D"], c["C"]
    rows = bad_rows(c)
    some = bool(rows.any())
    return dict(dlogits=rows[:, None].expand(B, C), rowloss=rows, loss=torch.tensor(some), gW=torch.full((C, D), some),
                gb=torch.full((C,), some), dybn=rows[:, None].expand(B, D),
                dfeat=torch.full((B, D), some) if training else rows[:, None].expand(B, D))


# ---------------------------------------------------------------------------------------------------------------- emulation
def group_sum(x):
    """column sums of x [B][D] in bn_fwd_kernel's order: row group g = b % 16 in row order, then the 16 partials in order"""
    B, D = x.shape
    nb = -(-B // 16)
    pad = torch.zeros(nb * 16, D, dtype=F32)
    pad[:B] = x
    pad = pad.view(nb, 16, D)
    s = torch.zeros(16, D, dtype=F32)
    for t in range(nb):
        s = s + pad[t]
    tot = torch.zeros(D, dtype=F32)
    for i in range(16):
        tot = tot + s[i]
    return tot


def product(A, Bm, K, seq):
    """sum_{k < K} A[:, k] Bm[:, k]: one product at a time in f32 (seq), or the float64 sum rounded once"""
    if not seq:
        return (A[:, :K].double() @ Bm[:, :K].double().T).float()
    acc = torch.zeros(A.shape[0], Bm.shape[0], dtype=F32)
    for k in range(K):
        acc = acc + A[:, k:k + 1] * Bm[:, k][None, :]
    return acc


def wave_order_sum(v):
    """loss_mean_kernel's order: lane l adds rows l, l + 64, ... in order, then an xor butterfly over the 64 lanes"""
    n = v.numel()
    nt = -(-n // 64)
    pad = torch.zeros(nt * 64, dtype=F32)
    pad[:n] = v
    pad = pad.view(nt, 64)
    s = torch.zeros(64, dtype=F32)
    for t in range(nt):
        s = s + pad[t]
    o = 32
    while o:
        s = s + s[torch.arange(64) ^ o]
        o >>= 1
    return s[0]


def tail_cut(K):
    return (K // 8) * 8


def head32(c, training, mut=None, rsq=0, seq=False):
    """the head in torch float32 with the kernels' rounding points; `mut` names one wrong head of the module docstring"""
    B, D, C = c["B"], c["D"], c["C"]
    feat, W, bias = c["feat"], c["W"], c["bias"]
    o = {}
    rm, rv = c["rm0"].clone(), c["rv0"].clone()
    if training or mut == "b":
        x = feat.clone()
        if mut == "c":
            x[-1] = 0
        bmean = group_sum(x) / float(B)
        t = feat - bmean
        if mut == "c":
            t = t.clone()
            t[-1] = 0
        qq = group_sum(t * t)
        bvar = qq / float(B)
        unbiased = qq / float(B - 1) if (B > 1 and mut != "a") else bvar
        rm = torch.tensor(0.9, dtype=F32) * rm + torch.tensor(0.1, dtype=F32) * bmean
        rv = torch.tensor(0.9, dtype=F32) * rv + torch.tensor(0.1, dtype=F32) * unbiased
    mean, var = (bmean, bvar) if training else (c["rm0"], c["rv0"])
    rstd = (1.0 / torch.sqrt((var + torch.tensor(1e-5, dtype=F32)).double())).float()
    if rsq:
        rstd = torch.nextafter(rstd, torch.full_like(rstd, float("inf") * rsq))
    ybn = (feat - mean) * rstd
    logits = product(ybn, W, tail_cut(D) if mut == "d_logits" else D, seq) + bias
    o.update(ybn=ybn, rstd=rstd, rm=rm, rv=rv, logits=logits)

    if c["targets"] is not None:
        y = c["targets"]
        n = torch.tensor(float(B) * float(C), dtype=F32)
        e = torch.exp(-logits.abs())
        l = logits.clamp(min=0) - logits * y + torch.log1p(e)
        sig = torch.where(logits >= 0, torch.ones_like(e), e) * (1.0 / (1.0 + e))
        dl = (sig - y) * (1.0 / n)
        loss = l.sum() / n
    else:
        lab = c["labels"]
        ign, bad = lab == IGNORE, bad_rows(c)
        nvalid = torch.tensor(float(B) if mut == "g" else float((~ign).sum()), dtype=F32)
        x = logits
        if mut == "k" and B > 128:
            x = logits.clone()
            x[128:] = logits[B - 1]
        m = x.max(1, keepdim=True).values
        ex = torch.exp(x - m)
        if mut == "i64":
            ex = ex[:, :64]
        if mut == "i128":
            ex = ex[:, :128]
        lse = m + torch.log(ex.sum(1, keepdim=True))
        safe = lab.clamp(0, C - 1)
        onehot = F.one_hot(safe, C).to(F32)
        dl = (torch.exp(x - lse) - onehot) / nvalid
        at_col = torch.minimum(safe ^ 64, torch.tensor(C - 1)) if (mut == "j" and C > 64) else safe
        rl = lse[:, 0] - x.gather(1, at_col[:, None])[:, 0]
        nanv = torch.tensor(float("nan"), dtype=F32)
        if mut != "h":
            dl = torch.where(ign[:, None], torch.zeros_like(dl), dl)
        dl = torch.where(bad[:, None], nanv, dl)
        rl = torch.where(ign, torch.zeros_like(rl), torch.where(bad, nanv, rl))
        loss = wave_order_sum(rl) / nvalid
        o["rowloss"] = rl
    o.update(dlogits=dl, loss=loss)
    Kb = tail_cut(B) if mut == "d_gw" else B
    gWg = product(dl.T.contiguous(), ybn.T.contiguous(), Kb, False)
    gbg = dl[:Kb].double().sum(0).float()
    o["gW"] = gWg if mut == "e" else c["gW0"] + gWg
    o["gb"] = gbg if mut == "f_over" else c["gb0"] + (gbg * float(-(-D // 32)) if mut == "f_tiles" else gbg)
    dy = product(dl, W.T.contiguous(), tail_cut(C) if mut == "d_dybn" else C, False)
    o["dybn"] = dy
    if training or mut == "m":
        m1 = group_sum(dy) / float(B)
        m2 = group_sum(dy * ybn) / float(B)
        o["dfeat"] = rstd * (dy - m1) if mut == "l" else rstd * (dy - m1 - ybn * m2)
    else:
        o["dfeat"] = rstd * dy
    o["dfeat_bf16"] = (bits(o["dfeat"]) & -65536).view(F32).to(BF) if mut == "n" else o["dfeat"].to(BF)
    return o


# ---------------------------------------------------------------------------------------------------------------- floors, gates
_FLOORS = {}


def forward_floors(c, training):
    """{output: max-rel of the emulation against float64}, the largest over rsqrtf off by -1, 0, +1 ulp"""
    key = (c["B"], c["D"], c["C"], c["variant"], bool(training))          # (the variant names the data: identity_pair's cases too)
    if key not in _FLOORS:
        r = head_ref(c, training)
        fl = dict.fromkeys(FWD_KEYS, 0.0)
        for rsq in (-1, 0, 1):
            e = head32(c, training, rsq=rsq, seq=True)
            for k in FWD_KEYS:
                fl[k] = max(fl[k], max_rel(e[k], r[k]))
        _FLOORS[key] = fl
    return _FLOORS[key]


def forward_gates(c, training):
    return {k: min(FWD_CAPS[k], FLOOR_FACTOR * max(v, ULP)) for k, v in forward_floors(c, training).items()}


def finite_max_rel(got, want, nan):
    """max-rel over the elements that are not expected to be NaN"""
    keep = ~nan
    if not bool(keep.any()):
        return 0.0
    return max_rel(got[keep], want[keep])


def figures(out, c, training):
    """{output: distance from the float64 reference} of whatever `out` holds: max-rel, absolute for the loss and the row losses"""
    r, nm = head_ref(c, training), nan_masks(c, training)
    fig = {}
    for k in FWD_KEYS + GRAD_KEYS:
        if k in out:
            fig[k] = finite_max_rel(out[k], r[k], nm.get(k, torch.zeros_like(r[k], dtype=torch.bool)))
    if "loss" in out and not bool(nm["loss"]):
        fig["loss"] = abs(float(out["loss"]) - float(r["loss"]))
    if "rowloss" in out and "rowloss" in r and not bool(nm["rowloss"].all()):
        keep = ~nm["rowloss"]
        fig["rowloss"] = float((out["rowloss"][keep].double() - r["rowloss"][keep]).abs().max())
    return fig


def check_head(out, c, training, label=""):
    """every assertion on one launch's outputs (CPU tensors; absent keys were not written by that form)"""
    r, nm, gates = head_ref(c, training), nan_masks(c, training), forward_gates(c, training)
    fig = figures(out, c, training)
    if label:
        t32 = figures(head_ref(c, training, F32), c, training)          # torch's own float32 head against float64, in brackets
        print(f"\n{label}: " + "  ".join(f"{k} {v:.2e} [{t32[k]:.1e}]" for k, v in fig.items()), end="")
    for k in FWD_KEYS:
        if k in out:
            assert out[k].shape == r[k].shape and bool(torch.isfinite(out[k]).all()), k
            assert fig[k] <= gates[k], (k, fig[k], gates[k])
    if not training:            # eval-mode BatchNorm leaves the running statistics alone, bit for bit
        for k, k0 in (("rm", "rm0"), ("rv", "rv0")):
            if k in out:
                assert torch.equal(bits(out[k]), bits(c[k0])), k
    for k in GRAD_KEYS + ("rowloss", "loss"):
        if k not in out or k not in nm or (k == "rowloss" and "rowloss" not in r):
            continue
        assert out[k].shape == r[k].shape, k
        assert torch.equal(torch.isnan(out[k]), nm[k]), f"{k}: NaN exactly where an out-of-range label reaches"
        assert bool(torch.isfinite(out[k][~nm[k]]).all()), k
        if k in fig:
            assert fig[k] < (LOSS_GATE if k in ("loss", "rowloss") else GRAD_GATE), (k, fig[k])
    if "dlogits" in out and c["labels"] is not None:          # an ignored row contributes nothing
        ign = c["labels"] == IGNORE
        assert float(out["dlogits"][ign].abs().sum()) == 0.0
        if "rowloss" in out:
            assert float(out["rowloss"][ign].abs().sum()) == 0.0
    if "dfeat_bf16" in out:
        want, keep = out["dfeat"].to(BF), ~torch.isnan(out["dfeat"])
        assert torch.equal(torch.isnan(out["dfeat_bf16"].float()), ~keep)
        assert torch.equal(bits(out["dfeat_bf16"])[keep], bits(want)[keep]), "dfeat_bf16 != round-to-nearest-even bf16 of dfeat"
    return fig


def check_identity(big, small):
    """the two-kernel cross entropy (B = 2049, last row ignored) against the one-workgroup kernel on the first 2048 rows"""
    assert torch.equal(bits(big["dlogits"][:2048]), bits(small["dlogits"]))
    assert float(big["dlogits"][2048].abs().sum()) == 0.0
    assert torch.equal(bits(big["rowloss"][:2048]), bits(small["rowloss"])) and float(big["rowloss"][2048]) == 0.0
    assert torch.equal(bits(big["loss"].reshape(1)), bits(small["loss"].reshape(1)))


# ---------------------------------------------------------------------------------------------------------------- tests
def runs():
    for shape in GRID:
        for variant in ("plain", "ignore"):
            yield shape, variant
    for shape in BCE_GRID:
        for variant in ("multihot", "soft"):
            yield shape, variant
    for shape in BAD_GRID:
        yield shape, "bad"


def test_labels_hold_both_halves_and_the_edges():
    for (B, D, C) in GRID:
        for variant in ("plain", "ignore"):
            lab = case(B, D, C, variant)["labels"]
            have = set(lab.tolist())
            for k in (0, 63, 64, C - 1):
                if k < C and B >= 8:
                    assert k in have, (B, D, C, variant, k)
            if B >= 136 and C > 64:          # (B = 129 has one row behind the first trip of the eight-row loop)
                assert bool((lab[128:] >= 64).any()) and bool(((lab[128:] >= 0) & (lab[128:] < 64)).any())
            if variant == "ignore" and B > 2:
                assert lab[0] == IGNORE and lab[B - 1] == IGNORE
    for (B, D, C) in BAD_GRID:
        lab = case(B, D, C, "bad")["labels"]
        assert lab[1] == C and lab[B - 1] == -1 and 0 <= lab[0] < C and int(bad_rows(case(B, D, C, "bad")).sum()) == 2


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B,D,C", GRID)
def test_emulation_passes_and_floors(B, D, C, training):
    """the unmutated emulation passes every assertion at every variant (and the one-product-at-a-time upper model, which the floors are
    measured with, the forward ones); prints the floors and the distance of torch's own float32 head from float64"""
    for variant in ("plain", "ignore"):
        c = case(B, D, C, variant)
        check_head(head32(c, training), c, training)
        upper = head32(c, training, seq=True)
        check_head({k: upper[k] for k in FWD_KEYS}, c, training)
    fl = forward_floors(c, training)
    t32 = figures({k: v.float() for k, v in head_ref(c, training, F32).items()}, c, training)
    print(f"\n({B},{D},{C}) {'train' if training else 'eval'}: floors " + "  ".join(f"{k} {v:.1e}" for k, v in fl.items()) +
          " | torch f32 vs f64 " + "  ".join(f"{k} {v:.1e}" for k, v in t32.items()), end="")
    for k, v in forward_gates(c, training).items():
        assert ULP * FLOOR_FACTOR <= v <= FWD_CAPS[k]
    for k in GRAD_KEYS:                                   # the project gates leave torch's own float32 room
        assert t32[k] < GRAD_GATE, (k, t32[k])
    assert t32["loss"] < LOSS_GATE        # (torch's float32 row losses: up to 2.3e-5 at (128,512,1000), 1.5e-5 at (64,768,397))


@pytest.mark.parametrize("training", [True, False])
def test_emulation_passes_bce_and_bad_labels(training):
    for shape in BCE_GRID:
        for variant in ("multihot", "soft"):
            c = case(*shape, variant)
            check_head(head32(c, training), c, training)
    for shape in BAD_GRID:
        c = case(*shape, "bad")
        out = head32(c, training)
        check_head(out, c, training)
        assert bool(torch.isnan(out["loss"])) and bool(torch.isnan(out["gW"]).all())
        ok_rows = ~bad_rows(c)
        assert bool(torch.isfinite(out["dlogits"][ok_rows]).all())


def test_identity_holds_for_the_emulation_and_sees_a_wrong_mean():
    for C in IDENTITY_C:
        big, small = identity_pair(C)
        check_identity(head32(big, False), head32(small, False))
        with pytest.raises(AssertionError):
            check_identity(head32(big, False, mut="g"), head32(small, False))
        with pytest.raises(AssertionError):
            check_identity(head32(big, False, mut="h"), head32(small, False))


def same_outputs(a, b):
    """the same values everywhere (NaN == NaN, +0 == -0: at C = 1 every gradient is a zero of one sign or the other)"""
    return all(bool(((a[k] == b[k]) | (torch.isnan(a[k].float()) & torch.isnan(b[k].float()))).all()) for k in a)


@pytest.mark.parametrize("mut", MUTANTS)
def test_every_mutant_fails_wherever_it_differs(mut):
    differs = 0
    for shape, variant in runs():
        c = case(*shape, variant)
        for training in (True, False):
            right, wrong = head32(c, training), head32(c, training, mut=mut)
            if same_outputs(right, wrong):
                continue
            differs += 1
            check_head(right, c, training)
            with pytest.raises(AssertionError):
                check_head(wrong, c, training)
    assert differs > 0, mut


def test_argument_struct_mirrors_the_header():
    """PevitHeadArgs names the members of pevit_head_args in the header's order, pointers as pointers and the rest int32; it carries
    every member of the launcher's HeadArgs"""
    import ctypes
    import os
    import re
    from conftest import ROOT
    from pevit_amd import _lib
    src = open(os.path.join(ROOT, "include", "pevit_hip.h")).read()
    body = re.search(r"typedef struct pevit_head_args \{(.*?)\} pevit_head_args;", src, flags=re.S).group(1)
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
    assert _lib.PevitHeadArgs._fields_ == members
    kern = open(os.path.join(ROOT, "pevit_amd", "csrc", "kernels.h")).read()
    launcher = re.search(r"struct HeadArgs \{(.*?)\n\};", kern, flags=re.S).group(1)
    launcher = re.sub(r"//.*", "", launcher)
    names = set(re.findall(r"(\w+)\s*=", launcher))
    assert names == {n for n, _ in members}
