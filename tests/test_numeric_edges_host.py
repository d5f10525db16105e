"""Host side of tests/test_gpu_numeric_edges.py (no GPU): the VALUE RANGE of the softmax, normalisation, loss and GELU kernels.

Every other kernel-level test feeds its kernel `randn` times a scale of order one.  This file states, on the CPU and with the kernel
nowhere in sight, the inputs at which such kernels go wrong (peaked, shifted, monotone, one-hot and uniform attention rows; rows whose
variance is at or below eps, rows far from zero, constant rows; logits of +-90 and more; pre-activations up to 16384), their float64
references, and for each regime

  * the floor: an emulation of the kernel's rounding points against float64 -- `attn_emul_bf16` for the attention core, the kernels'
    two-pass order in f32 for LayerNorm (`ln_emul`) and BatchNorm (`head32` of tests/test_head_host.py), the f32 formulas of the kernel
    comments for the losses (`head32` again) and for the GELU epilogues (`gelu_emul`);
  * the gate: an existing project gate wherever the floor is at most half of it (attention: out 1.5e-2, lse 2e-2, gradients rel-L2
    2e-2; LayerNorm: f32 1e-5 forward and 2e-5 backward, bf16 1e-2, column sums 1e-4; head: 2e-5 max-rel and 1e-5 absolute for the
    losses), else 4 x the floor of that regime, committed in FLOORS below (the emulation fixes the rounding points but not the f32
    summation order, hence the factor); where the true result is zero or vanishing (dQ / dK of one-hot and uniform rows, the
    mathematically zero dq[..., 63] of the offset regime) the gate is absolute, 4 x the emulation's max|emul - ref|, with the f32
    accumulator of dP modelled one product at a time (`attn_emul_f32acc`: in float64 arithmetic the two sums whose difference is dS
    cancel exactly) and that of attn_probs' S rounded once per 16-product matrix-core step (`probs_floor`);
  * the bite: named wrong kernels, each of which must exceed the gate of at least one regime of its family by 4x, or give NaN / inf:
        eps6, eps12     LayerNorm / BatchNorm with eps 1e-6, 1e-12          eps_out    eps added outside the square root
        onepass         variance as E[x^2] - mean^2                         pad0       padded keys at logit 0 instead of -3e38
        max0            the running maximum seeded with 0                   ce_nomax   cross entropy without the max subtraction
        bce_naive       BCE as log(1 + e^x) - x y                           tanh_e2u   tanh(u) as (e^2u - 1) / (e^2u + 1)

The emulation and the float64 code are the reference, never the kernel.  `pytest -s` prints every floor; the GPU file's docstring
records them next to what the MI355X measured.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F_

from conftest import max_rel
from pevit_amd import fp8
from test_head_host import GRAD_GATE as HEAD_GRAD_GATE, LOSS_GATE as HEAD_LOSS_GATE, RUNNING_GATE, head32, head_ref
from test_kernel_forms_host import GRAD_GATE, LSE_GATE, OUT_GATE, attn_emul_bf16, attn_ref64, deviations, heads_of, sweep_inputs

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
INF = float("inf")
BITE = 4.0                       # a wrong kernel must exceed the gate by this factor (or give NaN / inf)
MARGIN = 4.0                     # gate = MARGIN x committed floor where no existing gate fits

# Floors that exceed half of the existing gate, or that belong to an absolute gate: measured by this file (`pytest -s`), committed
# here, and re-checked by the tests below (the measured value must lie in [FLOOR / 2, FLOOR]).  key -> floor.
FLOORS = {
    ('attn', 'peaked1.5', 145, 'rowsum_exact'): 6.0e-06,      # measured 5.20e-06
    ('attn', 'peaked1.5', 257, 'rowsum_exact'): 7.8e-06,      # measured 6.74e-06
    ('attn', 'peaked4', 10, 'rowsum_exact'): 8.8e-06,      # measured 7.63e-06
    ('attn', 'peaked4', 50, 'rowsum_exact'): 1.5e-05,      # measured 1.23e-05
    ('attn', 'peaked4', 145, 'rowsum_exact'): 1.8e-05,      # measured 1.53e-05
    ('attn', 'peaked4', 257, 'rowsum_exact'): 1.8e-05,      # measured 1.53e-05
    ('attn', 'offset', 10, 'dq63'): 5.1e-01,      # measured 4.36e-01
    ('attn', 'offset', 10, 'rowsum_exact'): 6.4e-06,      # measured 5.48e-06
    ('attn', 'offset', 50, 'dq63'): 6.0e-01,      # measured 5.16e-01
    ('attn', 'offset', 50, 'rowsum_exact'): 1.1e-05,      # measured 9.37e-06
    ('attn', 'offset', 145, 'dq63'): 5.5e-01,      # measured 4.71e-01
    ('attn', 'offset', 145, 'rowsum_exact'): 1.3e-05,      # measured 1.06e-05
    ('attn', 'offset', 257, 'dq63'): 5.5e-01,      # measured 4.77e-01
    ('attn', 'offset', 257, 'rowsum_exact'): 1.4e-05,      # measured 1.14e-05
    ('attn', 'ramp', 145, 'rowsum_exact'): 6.9e-06,      # measured 5.93e-06
    ('attn', 'ramp', 257, 'rowsum_exact'): 1.3e-05,      # measured 1.09e-05
    ('attn', 'onehot', 10, 'lse'): 4.4e-06,      # measured 3.80e-06
    ('attn', 'onehot', 10, 'dq'): 6.1e-06,      # measured 5.28e-06
    ('attn', 'onehot', 10, 'dk'): 6.1e-06,      # measured 5.28e-06
    ('attn', 'onehot', 10, 'rowsum_exact'): 8.8e-06,      # measured 7.63e-06
    ('attn', 'onehot', 50, 'lse'): 4.4e-06,      # measured 3.80e-06
    ('attn', 'onehot', 50, 'dq'): 6.5e-06,      # measured 5.57e-06
    ('attn', 'onehot', 50, 'dk'): 6.5e-06,      # measured 5.57e-06
    ('attn', 'onehot', 50, 'rowsum_exact'): 8.8e-06,      # measured 7.63e-06
    ('attn', 'onehot', 145, 'lse'): 4.4e-06,      # measured 3.81e-06
    ('attn', 'onehot', 145, 'dq'): 7.5e-06,      # measured 6.44e-06
    ('attn', 'onehot', 145, 'dk'): 7.5e-06,      # measured 6.44e-06
    ('attn', 'onehot', 145, 'rowsum_exact'): 8.8e-06,      # measured 7.63e-06
    ('attn', 'onehot', 257, 'lse'): 4.4e-06,      # measured 3.81e-06
    ('attn', 'onehot', 257, 'dq'): 1.1e-05,      # measured 9.54e-06
    ('attn', 'onehot', 257, 'dk'): 1.1e-05,      # measured 9.54e-06
    ('attn', 'onehot', 257, 'rowsum_exact'): 8.8e-06,      # measured 7.63e-06
    ('attn', 'uniform', 10, 'dq'): 4.3e-02,      # measured 3.71e-02
    ('attn', 'uniform', 50, 'dq'): 3.3e-02,      # measured 2.80e-02
    ('attn', 'uniform', 145, 'dq'): 1.9e-02,      # measured 1.57e-02
    ('attn', 'uniform', 257, 'dq'): 1.8e-02,      # measured 1.56e-02
    ('ln', 'eps_offset', 128, 'y'): 1.6e-05,      # measured 1.36e-05
    ('ln', 'eps_offset', 768, 'y'): 1.5e-05,      # measured 1.28e-05
    ('ln', 'eps_offset', 1024, 'y'): 2.0e-05,      # measured 1.70e-05
    ('ln', 'offset1024', 128, 'y'): 3.9e-05,      # measured 3.37e-05
    ('ln', 'offset1024', 768, 'y'): 3.2e-05,      # measured 2.74e-05
    ('ln', 'offset1024', 1024, 'y'): 5.2e-05,      # measured 4.51e-05
    ('ln', 'offset1024', 1024, 'dgamma'): 6.0e-05,      # measured 5.19e-05
}


def gate_of(key, existing=None):
    """the gate of one figure: the existing project gate, or MARGIN x the committed floor of that regime"""
    if key in FLOORS:
        return MARGIN * FLOORS[key]
    assert existing is not None, key
    return existing


def check_floor(key, floor, existing=None):
    """the floor of one figure sits where its gate says: at most half of the existing gate, or inside [FLOOR / 2, FLOOR]"""
    if key in FLOORS:
        assert FLOORS[key] / 2 <= floor <= FLOORS[key], (key, floor, FLOORS[key])
    else:
        assert existing is not None and floor <= existing / 2, (key, floor, existing)


def bites(x, gate):
    return (not math.isfinite(x)) or x >= BITE * gate


def _bf(x):
    return x.to(BF).double()


# ======================================================================================================== 1. attention core
ATTN_BT, ATTN_H = 2, 3
ATTN_N = (10, 50, 145, 257)           # all-in-LDS family, runtime-N family, compile-time family; none a multiple of 32
CAUSAL_N = (17, 77)
ATTN_REGIMES = ("peaked1.5", "peaked4", "offset", "ramp", "onehot", "uniform")
CAUSAL_REGIMES = ("peaked1.5", "peaked4", "offset", "onehot")
DELTA_GEOMETRY = (6, 2, 10)           # Bt, H, N of the fused delta + attention launch (E = 128, six-head runs)
RAMP_SLOPE, RAMP_Q, RAMP_REST = 1.0 / 8, 4.0, 2.0 ** -7     # logit step 1/2 per key; the other 63 dimensions of q shrunk below it
ABS_REGIMES = {"onehot": ("dq", "dk"), "uniform": ("dq",)}        # gradients that vanish: absolute gates


def hot_key(N, causal=False):
    i = torch.arange(N)
    return (7 * i + 3) % (i + 1) if causal else (7 * i + 3) % N


def attn_inputs(regime, N, Bt=ATTN_BT, H=ATTN_H, causal=False):
    """q, k, v in the head layout (Bt*H, N, 64) and dO in the row layout (Bt*N, H*64), bf16: the sweep's recipe without the doubled
    last row, then modified per regime; every value is exact in bf16"""
    q, k, v, do = sweep_inputs(N, Bt, H, double_last=False)
    i = torch.arange(N)
    if regime.startswith("peaked"):                      # max|S| ~ 50 and ~150, mean row maximum of P 0.85 and 0.95
        q = (q.float() * (float(regime[6:]) / 0.35)).to(BF)
    elif regime == "offset":                             # every row of S shifted by 16 a_i in [-128, 128]
        k[..., 63] = 16.0
        q[..., 63] = ((i % 17) - 8).to(BF)
    elif regime == "ramp":                               # logits monotone in the key index, increasing / decreasing by query:
        q = (q.float() * RAMP_REST).to(BF)               # the row maximum sits on the last valid key, next to the padding, or on key 0
        k[..., 63] = (i * RAMP_SLOPE).to(BF)
        q[..., 63] = torch.where(i % 2 == 0, RAMP_Q, -RAMP_Q).to(BF)
    elif regime == "onehot":                             # q_i = k_h(i): the gap to the runner-up is at least 15
        q = k[:, hot_key(N, causal)].clone()
    elif regime == "uniform":                            # all keys of a head are equal: P = 1 / N
        k = k[:, :1].expand(-1, N, -1).contiguous()
    else:
        raise KeyError(regime)
    return q, k, v, do


def causal_fwd(q, k, v, emul=False):
    """float64 causal softmax attention (query x sees keys y <= x); emul: the kernels' rounding points (P in bf16 before the row sum
    and the product, out stored in bf16)"""
    q, k, v = q.double(), k.double(), v.double()
    N = q.shape[1]
    s = torch.bmm(q, k.transpose(1, 2))
    s = s.masked_fill(torch.triu(torch.ones(N, N, dtype=torch.bool), 1), -INF)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    if emul:
        e = _bf(e)
    out = torch.bmm(e, v) / e.sum(-1, keepdim=True)
    return _bf(out) if emul else out


def attn_emul_f32acc(q, k, v, do_heads):
    """attn_emul_bf16 with the f32 accumulators as further rounding points: S and delta = sum(dO * out) rounded to f32 once, dP = dO v^T
    one product at a time in f32 (the upper model of a matrix-core accumulator that tests/test_lowrank_host.py and test_head_host.py
    use).  Where a gradient vanishes (dS = P (dP - delta) with dP == delta in exact arithmetic: one-hot and uniform rows) the float64
    differences of attn_emul_bf16 are exact zeros and its floor says nothing about two f32 sums of the same terms in two orders;
    this one is the floor of the absolute gates."""
    q, k, v, do = q.double(), k.double(), v.double(), do_heads.double()
    s = torch.bmm(q, k.transpose(1, 2)).float().double()
    m = s.amax(dim=-1, keepdim=True)
    pb = _bf(torch.exp(s - m))
    l = pb.sum(dim=-1, keepdim=True)
    out = _bf(torch.bmm(pb, v) / l)
    lse = (m + torch.log(l)).float().double()
    delta = (do * out).sum(dim=-1, keepdim=True).float().double()
    p = torch.exp(s - lse).float().double()
    dp = torch.zeros(s.shape, dtype=F32)
    dof, vf = do.float(), v.float()
    for d in range(64):
        dp = dp + dof[:, :, None, d] * vf[:, None, :, d]
    dp = dp.double()
    dsb, pb2 = _bf((p * (dp - delta)).float()), _bf(p)
    return (out, lse.squeeze(-1), _bf(torch.bmm(dsb, k)), _bf(torch.bmm(dsb.transpose(1, 2), q)),
            _bf(torch.bmm(pb2.transpose(1, 2), do)))


def attn_wrong(q, k, v, what):
    """forward of a wrong kernel in f32 arithmetic: (out, lse).  pad0: the keys up to the next multiple of 32 enter the softmax with
    logit 0 (and v = 0); max0: the running maximum starts from 0, so exp(S - m) underflows on rows that lie far below zero"""
    s = torch.bmm(q.double(), k.double().transpose(1, 2)).float()
    vv = v.float()
    N = s.shape[-1]
    if what == "pad0":
        pad = -N % 32
        s = torch.cat([s, torch.zeros(*s.shape[:2], pad)], -1)
        vv = torch.cat([vv, torch.zeros(vv.shape[0], pad, 64)], 1)
        m = s.amax(-1, keepdim=True)
    elif what == "max0":
        m = s.amax(-1, keepdim=True).clamp_min(0.0)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    return (torch.bmm(e, vv) / l).double(), (m + torch.log(l)).squeeze(-1).double()


def probs_floor(q, k, lse64):
    """row sums of exp(S - lse) as attn_probs forms them: S from four chained v_mfma_f32_32x32x16_bf16 over d = 64 (attn_probs.hip),
    i.e. the f32 accumulator rounded once per 16 products (at |S| ~ 120 one f32 step of S is 7.6e-6 of P), lse in f32, the
    difference and the exponential in f32"""
    qd, kd = q.double(), k.double()
    s = torch.zeros(q.shape[0], q.shape[1], k.shape[1], dtype=F32)
    for d in range(0, 64, 16):
        s = (s.double() + torch.bmm(qd[..., d:d + 16], kd[..., d:d + 16].transpose(1, 2))).float()
    p = torch.exp(s - lse64.float().unsqueeze(-1))
    return float((p.double().sum(-1) - 1).abs().max())


ATTN_NAMES = ("out", "lse", "dq", "dk", "dv")
ATTN_GATES = dict(zip(ATTN_NAMES, (OUT_GATE, LSE_GATE, GRAD_GATE, GRAD_GATE, GRAD_GATE)))
ROWSUM_EXACT_TOL, ROWSUM_BF16_LSE_TOL = 1e-5, 2.1e-3       # tests/test_gpu_attention_seam.py


def attn_figures(got, ref, regime):
    """{name: figure} of (out, lse, dq, dk, dv) in the head layout: the five of `deviations`, with max|got - ref| in place of the
    rel-L2 for the gradients that vanish in this regime, and the mathematically zero dq[..., 63] of the offset regime"""
    fig = dict(zip(ATTN_NAMES, deviations(got, ref)))
    for n in ABS_REGIMES.get(regime, ()):
        i = ATTN_NAMES.index(n)
        fig[n] = float((got[i].double() - ref[i]).abs().max())
    if regime == "offset":
        fig["dq63"] = float((got[2][..., 63].double() - ref[2][..., 63]).abs().max())
    return fig


FLOOR_GATED = {("onehot", "lse")}           # lse of a one-hot row is S_hot: held to the f32 floor of S_hot, not to the 2e-2 of the sweep


def attn_gate(regime, N, name):
    key = ("attn", regime, N, name)
    return gate_of(key, ATTN_GATES.get(name))


@functools.lru_cache(maxsize=None)
def attn_case(regime, N, Bt=ATTN_BT, H=ATTN_H):
    q, k, v, do = attn_inputs(regime, N, Bt, H)
    doh = heads_of(do, Bt, H, N)
    return dict(q=q, k=k, v=v, do=do, ref=attn_ref64(q, k, v, doh), emul=attn_emul_bf16(q, k, v, doh),
                emul32=attn_emul_f32acc(q, k, v, doh))


@pytest.mark.parametrize("N", ATTN_N)
@pytest.mark.parametrize("regime", ATTN_REGIMES)
def test_attention_floors(regime, N):
    c = attn_case(regime, N)
    fig = attn_figures(c["emul"], c["ref"], regime)
    fig32 = attn_figures(c["emul32"], c["ref"], regime)
    for n in ABS_REGIMES.get(regime, ()) + ("dq63",):                # the absolute gates: the larger of the two emulations
        if n in fig:
            fig[n] = max(fig[n], fig32[n])
    s = torch.bmm(c["q"].double(), c["k"].double().transpose(1, 2))
    print(f"\nattn {regime:9s} N={N:3d} max|S| {float(s.abs().max()):6.1f} mean max P {float(torch.softmax(s, -1).amax(-1).mean()):.2f}  floor  "
          + "  ".join(f"{n} {x:.2e}" for n, x in fig.items()), end="")
    for n, x in fig.items():
        floor_only = n in ABS_REGIMES.get(regime, ()) or (regime, n) in FLOOR_GATED
        check_floor(("attn", regime, N, n), x, None if floor_only else ATTN_GATES.get(n))
    for lse, tol, name in ((c["ref"][1], ROWSUM_EXACT_TOL, "rowsum_exact"), (c["emul"][1], ROWSUM_BF16_LSE_TOL, "rowsum_kernel")):
        f = probs_floor(c["q"], c["k"], lse)
        print(f"  {name} {f:.2e}", end="")
        if name == "rowsum_kernel":              # 2.1e-3 is a bound, not a measurement: the row sum of bf16-rounded P is off by < 2^-9
            assert f < tol
        else:
            check_floor(("attn", regime, N, name), f, tol)
    if regime == "onehot":                       # out is v[h(i)] to the bit, for the emulation and for the rounded reference
        want = c["v"][:, hot_key(N)].double()
        gap = s.gather(-1, hot_key(N).expand(s.shape[0], N).unsqueeze(-1)).squeeze(-1) - \
            s.scatter(-1, hot_key(N).expand(s.shape[0], N).unsqueeze(-1), -INF).amax(-1)
        print(f"  smallest gap {float(gap.min()):.1f}", end="")
        assert float(gap.min()) >= 15
        assert torch.equal(c["emul"][0], want) and torch.equal(_bf(c["ref"][0]), want)
    if regime == "uniform":
        assert float(c["ref"][2].abs().max()) < 1e-12            # dQ vanishes
    if regime == "ramp":                         # every row of S is strictly monotone: increasing on even queries, decreasing on odd ones
        step = s[..., 1:] - s[..., :-1]
        up = (torch.arange(N) % 2 == 0)[None, :, None]
        assert bool(torch.where(up, step > 0, step < 0).all())
        assert torch.equal(s.argmax(-1), torch.where(up[..., 0], N - 1, 0).expand(s.shape[0], N))
        print(f"  smallest |step| {float(step.abs().min()):.2f}", end="")


@pytest.mark.parametrize("N", CAUSAL_N)
@pytest.mark.parametrize("regime", CAUSAL_REGIMES)
def test_causal_floors(regime, N):
    q, k, v, _ = attn_inputs(regime, N, causal=True)
    ref, emul = causal_fwd(q, k, v), causal_fwd(q, k, v, emul=True)
    f = max_rel(emul, ref)
    print(f"\ncausal {regime:9s} N={N:3d} floor out {f:.2e}", end="")
    check_floor(("causal", regime, N, "out"), f, OUT_GATE)
    assert torch.equal(emul[:, 0], v[:, 0].double()) and torch.equal(_bf(ref[:, 0]), v[:, 0].double())       # row 0 sees key 0 only
    if regime == "onehot":
        assert torch.equal(emul, v[:, hot_key(N, True)].double())


def test_delta_geometry_floor():
    Bt, H, N = DELTA_GEOMETRY
    for regime in ("peaked4", "offset"):
        c = attn_case(regime, N, Bt, H)
        fig = attn_figures(c["emul"], c["ref"], regime)
        print(f"\ndelta geometry {regime}: floor out {fig['out']:.2e} lse {fig['lse']:.2e}", end="")
        check_floor(("attn_delta", regime, N, "out"), fig["out"], OUT_GATE)
        check_floor(("attn_delta", regime, N, "lse"), fig["lse"], LSE_GATE)


def test_a_finite_mask_and_a_zero_seeded_maximum_are_seen():
    seen = {"pad0": [], "max0": []}
    for what in seen:
        for regime in ATTN_REGIMES:
            for N in ATTN_N:
                c = attn_case(regime, N)
                out, lse = attn_wrong(c["q"], c["k"], c["v"], what)
                e_out = max_rel(out, c["ref"][0]) if bool(torch.isfinite(out).all()) else INF
                e_lse = float((lse - c["ref"][1]).abs().max())
                e_lse = e_lse if math.isfinite(e_lse) else INF
                if bites(e_out, attn_gate(regime, N, "out")) and bites(e_lse, attn_gate(regime, N, "lse")):
                    seen[what].append((regime, N))
        print(f"\n{what}: out and lse beyond {BITE} x gate (or NaN) in {seen[what]}", end="")
    assert {r for r, _ in seen["pad0"]} >= {"offset"} and {r for r, _ in seen["max0"]} >= {"offset"}


# ======================================================================================================== 2. LayerNorm
LN_ROWS = 37
LN_WIDTHS = (128, 768, 1024)
LN_REGIMES = ("eps", "eps_offset", "offset64", "offset1024", "outlier", "constant")
LN_CONST = (0.0, 2.5, -1024.0)            # short mantissas: every partial sum of a constant row is exact
LN_F32_GATE, LN_BWD_GATE, LN_BF16_GATE, LN_COLSUM_GATE = 1e-5, 2e-5, 1e-2, 1e-4
LN_WRONG = ("eps6", "eps12", "eps_out", "onepass")
RSTD_CONST = 1.0 / math.sqrt(float(torch.tensor(1e-5, dtype=F32)))


def _r(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@functools.lru_cache(maxsize=None)
def ln_inputs(regime, E, rows=LN_ROWS):
    """x, gamma, beta, dy (f32), dy (bf16), dres (f32), dres (bf16)"""
    g, b = 1 + _r(E, seed=2, scale=0.2), _r(E, seed=3, scale=0.2)
    z = _r(rows, E, seed=1)
    if regime == "eps":
        x = 3e-3 * z                                   # variance ~ 1e-5 = eps
    elif regime == "eps_offset":
        x = 1e-3 * z + 0.5
    elif regime == "offset64":
        x = z + 64
    elif regime == "offset1024":
        x = z + 1024
    elif regime == "outlier":
        x = z.clone()
        x[:, 5] = 300.0
    elif regime == "constant":
        x = torch.tensor(LN_CONST)[torch.arange(rows) % 3][:, None].expand(rows, E).contiguous()
    else:
        raise KeyError(regime)
    dy, dres = _r(rows, E, seed=4), _r(rows, E, seed=5)
    return dict(x=x, g=g, b=b, dy=dy, dy16=dy.to(BF), dres=dres, dres16=dres.to(BF))


def lane_sum(vals):
    """row sums of [rows][E <= 1024] f32 in ln_fwd_kernel's order: lane l adds its float4 groups at columns 4 l + 256 i as
    ((x + y) + z) + w, group after group, then the xor butterfly over the 64 lanes (masked columns add 0)"""
    rows, E = vals.shape
    pad = torch.zeros(rows, 1024, dtype=F32)
    pad[:, :E] = vals
    g = pad.view(rows, 4, 64, 4)
    s = torch.zeros(rows, 64, dtype=F32)
    for i in range(4):
        s = s + (((g[:, i, :, 0] + g[:, i, :, 1]) + g[:, i, :, 2]) + g[:, i, :, 3])
    o = 32
    while o:
        s = s + s[:, torch.arange(64) ^ o]
        o >>= 1
    return s[:, 0]


def ln_emul(c, wrong=None, dy=None, dres=None):
    """LayerNorm forward and backward in f32 with the kernels' order (two passes; backward from the forward's mean and rstd)"""
    x, g, b = c["x"], c["g"], c["b"]
    E = x.shape[1]
    dy = c["dy"] if dy is None else dy.float()
    dres = c["dres"] if dres is None else dres.float()
    mean = lane_sum(x) / float(E)
    d = x - mean[:, None]
    var = lane_sum(x * x) / float(E) - mean * mean if wrong == "onepass" else lane_sum(d * d) / float(E)
    eps = torch.tensor({"eps6": 1e-6, "eps12": 1e-12}.get(wrong, 1e-5), dtype=F32)
    if wrong == "eps_out":
        rstd = (1.0 / (torch.sqrt(var.double()) + eps.double())).float()
    else:
        rstd = (1.0 / torch.sqrt((var + eps).double())).float()
    xh = d * rstd[:, None]
    y = xh * g + b
    gd = dy * g
    m1, m2 = lane_sum(gd) / float(E), lane_sum(gd * xh) / float(E)
    ln = rstd[:, None] * (gd - m1[:, None] - xh * m2[:, None])
    cs = [torch.zeros(E, dtype=F32) for _ in range(3)]
    for r in range(x.shape[0]):                        # column sums row after row in f32 (an upper model of the blocked order)
        cs[0], cs[1], cs[2] = cs[0] + dy[r] * xh[r], cs[1] + dy[r], cs[2] + dres[r]
    return dict(y=y, y16=y.to(BF), mean=mean, rstd=rstd, dx=ln + dres, dx16=(ln + dres).to(BF), dgamma=cs[0], dbeta=cs[1], dresum=cs[2])


def ln_ref(c, dy=None, dres=None):
    x, g, b = c["x"].double(), c["g"].double(), c["b"].double()
    dy = (c["dy"] if dy is None else dy).double()
    dres = (c["dres"] if dres is None else dres).double()
    mean = x.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((x - mean) ** 2).mean(-1, keepdim=True) + 1e-5)
    xh = (x - mean) * rstd
    gd = dy * g
    dx = rstd * (gd - gd.mean(-1, keepdim=True) - xh * (gd * xh).mean(-1, keepdim=True)) + dres
    return dict(y=xh * g + b, y16=xh * g + b, mean=mean[:, 0], rstd=rstd[:, 0], dx=dx, dx16=dx, dgamma=(dy * xh).sum(0), dbeta=dy.sum(0),
                dresum=dres.sum(0))


LN_EXISTING = dict(y=LN_F32_GATE, y16=LN_BF16_GATE, mean=LN_F32_GATE, rstd=LN_F32_GATE, dx=LN_BWD_GATE, dx16=LN_BF16_GATE,
                   dgamma=LN_COLSUM_GATE, dbeta=LN_COLSUM_GATE, dresum=LN_COLSUM_GATE)


def ln_figures(got, ref):
    return {k: max_rel(got[k].float(), ref[k]) for k in got if k in ref}


def ln_gate(regime, E, name):
    return gate_of(("ln", regime, E, name), LN_EXISTING[name])


@pytest.mark.parametrize("E", LN_WIDTHS)
@pytest.mark.parametrize("regime", LN_REGIMES)
def test_layernorm_floors(regime, E):
    c = ln_inputs(regime, E)
    e, r = ln_emul(c), ln_ref(c)
    fig = ln_figures(e, r)
    print(f"\nln {regime:10s} E={E:4d} floor  " + "  ".join(f"{n} {x:.2e}" for n, x in fig.items()), end="")
    for n, x in fig.items():
        check_floor(("ln", regime, E, n), x, LN_EXISTING[n])
    if regime == "constant":                  # exact: y = beta, mean = the row value, rstd = 1 / sqrt(f32(1e-5))
        assert torch.equal(e["y"], c["b"].expand_as(e["y"])) and torch.equal(e["mean"], c["x"][:, 0])
        assert float((e["rstd"].double() - RSTD_CONST).abs().max()) <= 2 * 2.0 ** -15          # 2 ulp at 316.2


def test_a_wrong_eps_and_a_one_pass_variance_are_seen():
    for wrong in LN_WRONG:
        seen = []
        for regime in LN_REGIMES:
            for E in LN_WIDTHS:
                c = ln_inputs(regime, E)
                fig = ln_figures(ln_emul(c, wrong), ln_ref(c))
                if fig["y"] >= BITE * ln_gate(regime, E, "y") and fig["dx"] >= BITE * ln_gate(regime, E, "dx"):
                    seen.append((regime, E, f"{fig['y']:.1e}"))
        print(f"\n{wrong}: y and dx beyond {BITE} x gate in {seen}", end="")
        assert seen, wrong
    # ... and none of them is seen at the inputs of test_layernorm_fwd_bwd (x = 2 randn + 0.5)
    c = dict(ln_inputs("eps", 768))
    c["x"] = 2.0 * _r(LN_ROWS, 768, seed=1) + 0.5
    for wrong in LN_WRONG:
        assert ln_figures(ln_emul(c, wrong), ln_ref(c))["y"] < LN_F32_GATE, wrong


# ======================================================================================================== 3. BatchNorm of the head
BN_SHAPE = (7, 64, 3)                     # B, D, C
BN_REGIMES = ("tiny_var", "const_col", "rv1e-6", "rv0")
BN_TRAINING = dict(tiny_var=True, const_col=True, **{"rv1e-6": False, "rv0": False})
BN_KEYS = ("ybn", "rstd", "rm", "rv", "logits", "dlogits", "dybn", "dfeat", "gW", "gb")


@functools.lru_cache(maxsize=None)
def bn_case(regime):
    """a case of tests/test_head_host.py (same keys: `head_ref`, `head32` and the GPU file's launcher take it)"""
    B, D, C = BN_SHAPE
    g = torch.Generator().manual_seed(77)

    def R(*s, sc=1.0):
        return torch.randn(*s, generator=g) * sc
    c = dict(B=B, D=D, C=C, variant="edge-" + regime, targets=None)
    c["feat"] = R(B, D, sc=1.5) + 0.3
    c["W"], c["bias"] = R(C, D, sc=0.2), R(C, sc=0.2)
    c["rm0"], c["rv0"] = R(D, sc=0.1), R(D, sc=0.1).abs() + 0.5
    c["gW0"], c["gb0"] = R(C, D, sc=0.05), R(C, sc=0.05)
    c["labels"] = torch.tensor([0, 2, 1, 1, 0, 2, 1])
    if regime == "tiny_var":              # every second column: batch variance ~ 1e-5 = eps (the offset is small: at 0.5 the spacing
        c["feat"][:, ::2] = 3e-3 * R(B, D // 2) + 2.0 ** -6        # of the inputs themselves puts the ybn floor at 6.5e-6)
    elif regime == "const_col":           # columns constant over the batch, with short mantissas: the batch variance is exactly 0
        c["feat"][:, 0], c["feat"][:, 5], c["feat"][:, D - 1] = 0.0, 2.5, -1024.0
    elif regime == "rv1e-6":
        c["rv0"][::2] = 1e-6
    elif regime == "rv0":
        c["rv0"][::2] = 0.0
    return c


def head_wrong_eps(c, training, wrong):
    """ybn and rstd of a BatchNorm with a wrong eps, in float64 (the rest of the head follows from them)"""
    f = c["feat"].double()
    mean, var = (f.mean(0), f.var(0, unbiased=False)) if training else (c["rm0"].double(), c["rv0"].double())
    eps = {"eps6": 1e-6, "eps12": 1e-12}.get(wrong, 1e-5)
    rstd = 1.0 / (torch.sqrt(var) + eps) if wrong == "eps_out" else 1.0 / torch.sqrt(var + eps)
    return dict(ybn=(f - mean) * rstd, rstd=rstd)


def head_figures(got, ref, keys):
    fig = {k: max_rel(got[k], ref[k]) for k in keys if k in got}
    if "loss" in got:
        fig["loss"] = abs(float(got["loss"]) - float(ref["loss"]))
    if "rowloss" in got and "rowloss" in ref:
        fig["rowloss"] = float((got["rowloss"].double() - ref["rowloss"]).abs().max())
    return fig


def head_existing(name):
    """the head's gates: 1e-5 absolute for the losses, 1e-6 for the running statistics, 2e-5 max-rel for everything else"""
    return HEAD_LOSS_GATE if name in ("loss", "rowloss") else RUNNING_GATE if name in ("rm", "rv") else HEAD_GRAD_GATE


def head_gate(section, regime, name):
    return gate_of((section, regime, name), head_existing(name))


@pytest.mark.parametrize("regime", BN_REGIMES)
def test_batchnorm_floors(regime):
    c, training = bn_case(regime), BN_TRAINING[regime]
    r = head_ref(c, training)
    e = head32(c, training)
    fig = head_figures({k: e[k] for k in BN_KEYS}, r, BN_KEYS)
    print(f"\nbn {regime:9s} floor  " + "  ".join(f"{n} {x:.2e}" for n, x in fig.items()), end="")
    for n, x in fig.items():
        check_floor(("bn", regime, n), x, head_existing(n))
    seen = [w for w in ("eps6", "eps12", "eps_out")
            if any(max_rel(head_wrong_eps(c, training, w)[k], r[k]) >= BITE * head_gate("bn", regime, k) for k in ("ybn", "rstd"))]
    print(f"  wrong eps seen: {seen}", end="")
    assert len(seen) == 3


# ======================================================================================================== 4. losses
LOSS_SHAPES = ((7, 64, 3), (33, 160, 130), (2050, 16, 5))      # one workgroup; C > 128: slices and a tail; two kernels beyond 2048 rows
CE_ROWS = ("all+90", "all-90", "hot_on", "hot_off", "equal", "plain")
BCE_LOGITS = (100.0, -100.0, 30.0, -30.0, 0.0, -0.0, 1e-30)
BCE_TARGETS = (0.0, 1.0, 0.25, 0.8125)
IGNORE = -100


def selection_head(B, D, C, logits, variant, biased=True):
    """a head whose logits ARE `logits`, exactly: eval mode, running mean 0, running variance 1 - 1e-5 (rstd == 1), W a 0/1
    selection matrix, small integer biases (none where a logit of 1e-30 would be lost in the sum)"""
    c = dict(B=B, D=D, C=C, variant=variant, labels=None, targets=None)
    c["bias"] = ((torch.arange(C) % 3) - 1).float() if biased else torch.zeros(C)
    c["feat"] = torch.zeros(B, D)
    c["feat"][:, :C] = logits - c["bias"]
    c["feat"][:, C:] = 0.5
    assert torch.equal(c["feat"][:, :C] + c["bias"], logits)
    c["W"] = torch.eye(C, D)
    c["rm0"], c["rv0"] = torch.zeros(D), torch.full((D,), 1.0) - 1e-5
    assert bool((c["rv0"] + torch.tensor(1e-5) == 1.0).all())
    c["gW0"], c["gb0"] = torch.zeros(C, D), torch.zeros(C)
    c["want_logits"] = logits
    return c


@functools.lru_cache(maxsize=None)
def ce_case(B, D, C, all_ignored=False):
    logits, labels = torch.zeros(B, C), torch.zeros(B, dtype=torch.int64)
    z = _r(B, C, seed=B + C).to(BF).float()
    for b in range(B):
        kind, hot = CE_ROWS[b % len(CE_ROWS)], (5 * b + 1) % C
        labels[b] = hot
        if kind == "all+90":
            logits[b] = 90.0
        elif kind == "all-90":
            logits[b] = -90.0
        elif kind in ("hot_on", "hot_off"):
            logits[b, hot] = 80.0
            if kind == "hot_off":
                labels[b] = (hot + 1) % C
        elif kind == "equal":
            logits[b] = 3.5
        else:
            logits[b] = z[b]
    if all_ignored:
        labels[:] = IGNORE
    c = selection_head(B, D, C, logits, "edge-ce-ignored" if all_ignored else "edge-ce")
    c["labels"] = labels
    return c


@functools.lru_cache(maxsize=None)
def bce_case(B, D, C):
    n = torch.arange(B * C)
    logits = torch.tensor(BCE_LOGITS)[n % len(BCE_LOGITS)].view(B, C)
    c = selection_head(B, D, C, logits, "edge-bce", biased=False)
    c["targets"] = torch.tensor(BCE_TARGETS)[(n // len(BCE_LOGITS)) % len(BCE_TARGETS)].view(B, C)
    return c


def loss_ref(c):
    """float64: cross entropy from log_softmax, BCE as max(x, 0) - x y + log1p(e^-|x|) and sigma - y"""
    x = c["want_logits"].double()
    if c["targets"] is not None:
        y = c["targets"].double()
        l = x.clamp(min=0) - x * y + torch.log1p(torch.exp(-x.abs()))
        return dict(loss=l.mean(), dlogits=(torch.sigmoid(x) - y) / x.numel())
    lab = c["labels"]
    valid = lab != IGNORE
    ls = torch.log_softmax(x, -1)
    rl = torch.where(valid, -ls.gather(1, lab.clamp(min=0)[:, None])[:, 0], torch.zeros(x.shape[0], dtype=F64))
    nv = float(valid.sum())
    onehot = F_.one_hot(lab.clamp(min=0), x.shape[1]).double()
    dl = torch.where(valid[:, None], (ls.exp() - onehot) / max(nv, 1.0), torch.zeros_like(x))
    return dict(rowloss=rl, loss=rl.sum() / nv if nv else torch.tensor(float("nan"), dtype=F64), dlogits=dl)


def loss_wrong(c, what):
    """the loss of a wrong kernel in f32: ce_nomax = log(sum e^x) without the max subtraction; bce_naive = log(1 + e^x) - x y"""
    x = c["want_logits"]
    if what == "bce_naive":
        return float((torch.log(1 + torch.exp(x)) - x * c["targets"]).mean())
    lse = torch.log(torch.exp(x).sum(-1))
    return float((lse - x.gather(1, c["labels"][:, None])[:, 0]).mean())


@pytest.mark.parametrize("B,D,C", LOSS_SHAPES)
def test_loss_floors(B, D, C):
    for c, name in ((ce_case(B, D, C), "ce"), (bce_case(B, D, C), "bce")):
        e, r = head32(c, False), loss_ref(c)
        assert torch.equal(e["logits"], c["want_logits"]) and bool((e["rstd"] == 1).all())          # the head's logits ARE the stated ones
        r = dict(r, gW=r["dlogits"].T @ c["feat"].double(), gb=r["dlogits"].sum(0))          # (ybn == feat: what the probe's step returns)
        fig = head_figures(e, r, ("dlogits", "gW", "gb"))
        print(f"\n{name} ({B},{D},{C}) floor  " + "  ".join(f"{n} {x:.2e}" for n, x in fig.items()), end="")
        for n, x in fig.items():
            check_floor((name, (B, D, C), n), x, head_existing(n))
        # torch's own functions agree with the formulas above
        x = c["want_logits"].double()
        t = F_.cross_entropy(x, c["labels"]) if name == "ce" else F_.binary_cross_entropy_with_logits(x, c["targets"].double())
        assert abs(float(t) - float(r["loss"])) < 1e-12
        w = loss_wrong(c, "ce_nomax" if name == "ce" else "bce_naive")
        print(f"  wrong loss {w}", end="")
        assert not math.isfinite(w)


def test_all_rows_ignored_is_what_torch_returns():
    """F.cross_entropy over a batch whose rows are all ignore_index: the mean over zero rows, NaN, and a zero gradient"""
    c = ce_case(*LOSS_SHAPES[0], all_ignored=True)
    x = c["want_logits"].double().requires_grad_(True)
    loss = F_.cross_entropy(x, c["labels"])
    loss.backward()
    assert math.isnan(float(loss.detach())) and float(x.grad.abs().max()) == 0.0
    r, e = loss_ref(c), head32(c, False)
    assert math.isnan(float(r["loss"])) and float(r["dlogits"].abs().max()) == 0.0
    assert math.isnan(float(e["loss"])) and float(e["dlogits"].abs().max()) == 0.0


# ======================================================================================================== 5. GELU epilogues
GELU_MAGS = (0.5, 3.0, 10.0, 30.0, 52.0, 53.0, 60.0, 100.0, 16384.0)
GELU_GATE = 1e-2                           # the bf16 gate, here per element
BF16_SUBNORMAL_STEP = 2.0 ** -133
GELU_KINDS = ("quick", "dquick", "new", "dnew")
_C0, _C1 = 0.7978845608028654, 0.044715


def gelu_grid():
    """the pre-activations, exact in bf16: +-0, +-1e-30 (rounded to bf16), +-GELU_MAGS"""
    tiny = float(torch.tensor(1e-30).to(BF))
    vals = [0.0, -0.0, tiny, -tiny]
    for m in GELU_MAGS:
        vals += [m, -m]
    g = torch.tensor(vals, dtype=F32)
    assert torch.equal(g.to(BF).float(), g)
    return g


def gelu_ref(kind, x):
    x = x.double()
    if kind in ("quick", "dquick"):
        s = torch.sigmoid(1.702 * x)
        return x * s if kind == "quick" else s * (1 + 1.702 * x * (1 - s))
    u = _C0 * (x + _C1 * x ** 3)
    th = torch.tanh(u)
    return 0.5 * x * (1 + th) if kind == "new" else 0.5 * (1 + th) + 0.5 * x * (1 - th * th) * _C0 * (1 + 3 * _C1 * x * x)


def gelu_emul(kind, x, wrong=None):
    """the f32 formulas of gemm_epilogue.h: sigmoid as 1 / (1 + 2^(-log2(e) x)), gelu_new from tanhf; the result stored in bf16"""
    x = x.float()
    if kind in ("quick", "dquick"):
        s = 1.0 / (1.0 + torch.exp2(torch.tensor(-1.4426950408889634, dtype=F32) * (torch.tensor(1.702, dtype=F32) * x)))
        out = x * s if kind == "quick" else s * (1.0 + torch.tensor(1.702, dtype=F32) * x * (1.0 - s))
        return out.to(BF)
    u = torch.tensor(_C0, dtype=F32) * (x + torch.tensor(_C1, dtype=F32) * x * x * x)
    if wrong == "tanh_e2u":
        e = torch.exp(2 * u)
        th = (e - 1) / (e + 1)
    else:
        th = torch.tanh(u)
    if kind == "new":
        return (0.5 * x * (1.0 + th)).to(BF)
    return (0.5 * (1.0 + th) + 0.5 * x * (1.0 - th * th) * torch.tensor(_C0, dtype=F32) * (1.0 + 3.0 * torch.tensor(_C1, dtype=F32) * x * x)).to(BF)


def gelu_abs_term(x):
    """the absolute term of the GELU gate: one bf16 subnormal step, and where the f32 sigmoid itself leaves the normal range,
    (1 + 2|x|) 2^-126.  The sigmoid is formed in f32 as 1 / (1 + 2^t): from t = 128 on (x = -53) the power is inf and the quotient 0 in
    exact IEEE f32 arithmetic already, and a hardware reciprocal may flush every quotient below the smallest normal 2^-126 (x = -52).
    The value and the derivative multiply that sigmoid by x and by 1 + 1.702 x (1 - s): what is lost is at most (1 + 2|x|) 2^-126,
    6e-37 at |x| = 53 -- test_gelu_floors shows that the f32 formula on the CPU misses the one-subnormal-step term alone at x = -53."""
    return torch.maximum(torch.tensor(BF16_SUBNORMAL_STEP, dtype=F64), (1 + 2 * x.double().abs()) * 2.0 ** -126)


def gelu_check(kind, got, x):
    """got (bf16) against float64 at the pre-activations x: per element within 1e-2 relative plus gelu_abs_term, finite, and exactly
    x / exactly +-0 where the bf16-rounded reference is.  Returns the largest relative deviation."""
    x, got = x.reshape(-1), got.reshape(-1)
    ref = gelu_ref(kind, x)
    g = got.double()
    assert bool(torch.isfinite(got.float()).all()), (kind, "NaN or inf")
    excess = (g - ref).abs() - (GELU_GATE * ref.abs() + gelu_abs_term(x))
    assert float(excess.max()) <= 0, (kind, x[excess.argmax()], got[excess.argmax()], ref[excess.argmax()])
    rb = ref.to(BF)
    ident = rb.float() == x.float()
    if kind in ("quick", "new"):
        assert torch.equal(got[ident].view(torch.int16), x[ident].to(BF).view(torch.int16)), (kind, "not exactly x")
    zero = rb.float() == 0
    assert torch.equal(got[zero].view(torch.int16), rb[zero].view(torch.int16)), (kind, "not exactly +-0")
    nz = ref.abs() > 1e-30
    return float(((g - ref).abs()[nz] / ref.abs()[nz]).max())


@pytest.mark.parametrize("kind", GELU_KINDS)
def test_gelu_floors(kind):
    x = gelu_grid()
    f = gelu_check(kind, gelu_emul(kind, x), x)
    print(f"\ngelu {kind:6s} floor (largest relative deviation of the f32 formula stored in bf16) {f:.2e}", end="")
    assert f <= GELU_GATE / 2
    if kind in ("new", "dnew"):
        bad = gelu_emul(kind, x, "tanh_e2u")
        print(f"  tanh from e^2u: {int(torch.isnan(bad.float()).sum())} NaN of {x.numel()}", end="")
        assert bool(torch.isnan(bad.float()).any())
        with pytest.raises(AssertionError):
            gelu_check(kind, bad, x)


# ======================================================================================================== 6. fp8 row scales
FP8_SHAPE = (128, 128)


@functools.lru_cache(maxsize=None)
def fp8_rows():
    """rows whose amax sits on, just above and just below 448 2^k; an all-zero row; a single non-zero element"""
    rows, cols = FP8_SHAPE
    w = _r(rows, cols, seed=9)
    w = w / w.abs().amax(1, keepdim=True) * 0.99            # |w| < 1 everywhere, then one element per row sets amax
    kinds = []
    for r in range(rows):
        k = (r % 13) - 6
        edge = torch.tensor(448.0 * 2.0 ** k, dtype=F32)
        kind = r % 5
        if kind < 3:
            amax = (edge, torch.nextafter(edge, torch.tensor(INF)), torch.nextafter(edge, torch.tensor(0.0)))[kind]
            w[r] = w[r] * amax * 0.5
            w[r, (7 * r) % cols] = amax if r % 2 else -amax
        elif kind == 3:
            w[r] = 0.0
        else:
            w[r] = 0.0
            w[r, (11 * r) % cols] = float(edge) * 0.3
        kinds.append(kind)
    return w, kinds


def test_fp8_boundary_rows_on_the_host_packer():
    w, kinds = fp8_rows()
    codes, scales = fp8.quantize_rows(w)
    assert not bool(((codes & 0x7F) == 0x7F).any())          # no code is the NaN pattern
    amax = w.abs().amax(1)
    for r, kind in enumerate(kinds):
        if kind == 0:
            assert float(amax[r] / scales[r]) == 448.0
        elif kind == 1:
            assert 224.0 < float(amax[r] / scales[r]) < 224.001
        elif kind == 2:
            assert 447.99 < float(amax[r] / scales[r]) < 448.0
        elif kind == 3:
            assert float(scales[r]) == 1.0 and int(codes[r].max()) == 0
    assert float((fp8.dequantize_rows(codes, scales) - w).abs().max()) <= float((amax / 14).max())
