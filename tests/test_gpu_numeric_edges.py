"""The softmax, normalisation, loss and GELU kernels at the edges of their VALUE range, one kernel at a time through the C ABI.

Inputs, float64 references, floors, gates and the proof that the gates bite come from tests/test_numeric_edges_host.py; nothing here
is compared with another kernel's output except where a bit-for-bit identity is the claim.  Every output is pre-filled with NaN and
followed by a guard that must survive; every element of every output enters its comparison.

Gates: an existing project gate where the CPU floor is at most half of it, else 4 x the floor committed in FLOORS of the host file
(marked * below); `pytest -s` prints every figure next to its gate.  CPU floor | measured on the MI355X, ranges over the sizes:

 1. attention core, Bt = 2, H = 3, N in {10, 50, 145, 257} (gates: out 1.5e-2 max-rel, lse 2e-2, dQ / dK / dV 2e-2 rel-L2)
      regime      out                  lse                  dQ                   dK                   dV
      peaked1.5   2.0e-3..3.2e-3 | same  8.3e-4..1.5e-3 | same  5.5e-3..6.3e-3 | 2.2e-3..6.1e-3  5.3e-3..6.9e-3 | 2.5e-3..5.8e-3  2.0e-3..2.1e-3 | same
      peaked4     1.9e-3..2.4e-3 | same  6.1e-4..1.2e-3 | same  6.2e-3..7.9e-3 | 2.2e-3..6.8e-3  5.8e-3..9.3e-3 | 2.4e-3..6.4e-3  1.5e-3..1.8e-3 | same
      offset      2.3e-3..2.6e-3 | same  1.1e-3..1.4e-3 | same  6.9e-3..8.0e-3 | 4.4e-3..7.3e-3  2.7e-3..3.3e-3 | 2.2e-3..2.7e-3  2.3e-3..2.4e-3 | same
                  max|dq[..., 63]| (mathematically 0) *: 4.4e-1..5.2e-1 | 2.3e-1..4.8e-1
      ramp        2.0e-3..3.3e-3 | same  1.2e-3..1.5e-3 | same  2.8e-3..8.7e-3 | 2.5e-3..8.6e-3  2.2e-3..2.9e-3 | 2.2e-3..2.9e-3  2.2e-3..2.3e-3 | same
                  (every row of S strictly monotone, step >= 0.35 per key: the row maximum is key N - 1 on even queries, key 0 on odd ones)
      onehot      out == v[h(i)] bit for bit at every N; lse *: 3.8e-6 | 6.4e-6..1.0e-5 (S_hot ~ 100 from an f32 accumulator);
                  max|dQ|, max|dK| *: 5.3e-6..9.5e-6 | 7.0e-12..1.1e-5;  dV 2.1e-12..2.1e-8 | same
      uniform     1.5e-3..2.6e-3 | same  3.9e-7..4.8e-7 | 3.9e-7..1.7e-6  max|dQ| *: 1.6e-2..3.7e-2 | 1.6e-2..2.5e-2  dK 2.4e-3 | 2.3e-3..2.4e-3
                  dV 1.6e-3..2.0e-3 | same
    attn_probs row sums, |sum - 1|: with the exact lse (1e-5, or * where the floor of an f32 S passes 5e-6: then 5.2e-6..1.5e-5)
      2.3e-7..1.5e-5 | 1.6e-7..2.4e-5, worst against its gate offset N = 10, 1.7e-5 of 2.6e-5; with the kernel's lse (2.1e-3 = the
      bound 2^-9 of the bf16 row sum) 4.6e-7..1.5e-3 | 1.1e-11..1.5e-3.  No NaN, no inf, no negative probability in any regime.
    causal, N in {17, 77}: out 1.9e-3..2.6e-3 | the same to two digits; one-hot rows and row 0 of every regime bit for bit.
    fused delta + attention at (Bt, H, N) = (6, 2, 10), peaked4 / offset: out 2.0e-3 / 2.5e-3 | 2.0e-3 / 2.5e-3, lse 6.1e-4 / 1.3e-3 |
      6.0e-4 / 1.3e-3; the bits of attn_fwd on the same operands.
 2. LayerNorm, 37 rows, E in {128, 768, 1024}: ln_fwd, ln_bwd, ln_bwd_ex (bf16 dy and residual), ln_bwd_affine
      regime       y (1e-5)                       dx (2e-5)                  d gamma (1e-4)              bf16 outputs (1e-2)
      eps          8.4e-8..1.2e-7 | 6.9e-8..1.0e-7  1.0e-7..1.4e-7 | 9.3e-8..1.6e-7  1.8e-7..2.0e-7 | 5.7e-8..1.4e-7   2.0e-3..3.5e-3 | same
      eps_offset * 1.3e-5..1.7e-5 | same           1.5e-7..4.8e-7 | same             1.4e-5..2.2e-5 | same             2.2e-3..3.0e-3 | same
      offset64     1.4e-6..1.9e-6 | same           1.2e-7..5.1e-7 | 1.2e-7..5.3e-7   1.9e-6..2.6e-6 | 1.9e-6..2.5e-6   1.4e-3..3.0e-3 | same
      offset1024 * 2.7e-5..4.5e-5 | same           2.5e-6..8.2e-6 | same             3.2e-5..5.2e-5 (* at 1024) | same 1.4e-3..3.0e-3 | same
      outlier      1.3e-7..2.0e-7 | 1.5e-7..2.0e-7  3.2e-8..4.0e-8 | 3.2e-8..4.6e-8  6.6e-8..4.2e-6 | 9.8e-8..4.3e-6   1.6e-3..2.4e-3 | same
      constant     y == beta, mean == the row value, bit for bit; rstd 5.4e-8 | 4.2e-8 (within 2 ulp of 1 / sqrt(1e-5f)); dx 1.4e-7..2.1e-7 | 8.7e-8..1.3e-7
      mean and rstd (1e-5): at most 1.6e-7 on both sides; d beta and the residual column sum at most 2.5e-7 | 1.4e-7.
    the LayerNorm inside adapter_fwd_kernel (E = 768, T = 37), floors = those of y in bf16, mean and rstd at E = 768: z 1.6e-3..3.0e-3 |
      the same to three digits, mean 0..1.4e-7 | same, rstd 5.0e-8..1.4e-7 | 4.2e-8..1.4e-7; constant rows exact.
 3. BatchNorm, (B, D, C) = (7, 64, 3) (2e-5 max-rel; running statistics 1e-6): tiny batch variance, a constant column (training),
    running variance 1e-6 and 0 (eval).  ybn 7.6e-8..1.5e-7 | 6.7e-8..1.5e-7, rstd 2.6e-8..5.6e-8 | same, running statistics
    <= 1.2e-7 | same, dfeat 5.7e-8..1.4e-7 | 4.0e-8..1.9e-7, logits / dlogits / dybn / gW / gb <= 4.4e-7 | <= 5.3e-7.
    The probe (pevit_probe_step, pevit_probe_predict) on the same cases, floors = those of the head's emulation: logits 4.4e-8..2.8e-7 |
    2.2e-7..3.4e-7, gW 9.9e-8..1.8e-7 | 5.9e-8..1.6e-7, gb 5.4e-8..4.4e-7 | 4.5e-8..4.1e-7, running statistics <= 1.2e-7 | <= 1.2e-7.
 4. losses at logits that ARE the stated ones (asserted first), shapes (7,64,3), (33,160,130), (2050,16,5); gates 2e-5 / 1e-5 absolute
      cross entropy (all +90, all -90, one logit 80 above the rest with the label on / off it, all equal, plain):
        dlogits 3.1e-8..7.9e-7 | 4.8e-8..8.2e-7   loss 3.0e-7..1.4e-6 | 3.0e-7..1.4e-6   row losses 1.9e-6..4.0e-6 | 1.9e-6..3.6e-6
      BCE (logits +-100, +-30, +-0, 1e-30 x targets 0, 1, 0.25, 0.8125): dlogits 3.3e-8..5.9e-8 | same   loss 2.2e-8..2.9e-6 | 2.2e-8..6.7e-6
      all rows ignore_index: loss NaN (torch's answer: a mean over zero rows), dlogits and row losses exactly 0.
      the probe's own loss code at (7,64,3), (33,160,130): loss 2.2e-8..1.4e-6 | 2.2e-8..1.4e-6, gW 3.5e-8..4.9e-7 | 6.3e-8..1.3e-7,
        gb 3.4e-8..3.4e-6 | 4.5e-8..1.4e-7.
 5. GELU epilogues at +-0, +-1e-30, +-{0.5, 3, 10, 30, 52, 53, 60, 100, 16384}, per element 1e-2 relative + gelu_abs_term:
      QuickGELU 3.1e-3 | 3.1e-3, its derivative 2.8e-3 | 2.8e-3, gelu_new 1.6e-3 | 1.6e-3, its derivative 3.7e-3 | 3.7e-3 (gemm_ex and
      the fused adapter kernels alike); DRELU at aux = +-0 gives +0; no NaN, no inf; exactly x / exactly +-0 where the reference is.
 6. fp8 row scales at amax = 448 2^k and its two neighbours, zero rows, single elements: scales, codes and the dequantised values of
    pevit_amd/fp8.py, no NaN code.
"""
import ctypes as C
import functools

import pytest
import torch

from conftest import max_rel
from test_gpu_kernel_forms import NAN, P, S, guard_intact, guarded, ok, same_bits
from test_kernel_forms_host import heads_of
import test_numeric_edges_host as H

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pevit_amd import _lib
    return _lib.load()


def say(tag, fig, gates):
    """prints every figure next to its gate, then asserts all of them"""
    print(f"\n{tag}: " + "  ".join(f"{k} {v:.2e} ({gates[k]:.1e})" for k, v in fig.items()), end="")
    for k, v in fig.items():
        assert v <= gates[k], (tag, k, v, gates[k])


def finite(*ts):
    return all(bool(torch.isfinite(t.float()).all()) for t in ts)


# ======================================================================================================== 1. attention core
@functools.lru_cache(maxsize=None)
def attn_gpu(regime, N, Bt=H.ATTN_BT, Hh=H.ATTN_H):
    """operands on the GPU and the float64 reference in the head layout, computed once and shared: the kernels that take them read
    them only; the one launch that writes its operands (attn_fwd_delta) gets clones"""
    c = H.attn_case(regime, N, Bt, Hh)
    return dict(q=c["q"].cuda(), k=c["k"].cuda(), v=c["v"].cuda(), do=c["do"].cuda(), ref=c["ref"])


def attn_fwd(lib, c, Bt, Hh, N):
    """pevit_op_attn_fwd with and without the lse store: (out rows bf16, lse (Bt*H, N) f32), guards checked"""
    E, T = Hh * 64, Bt * N
    out, out_inf = guarded(T, E, BF, E + 8), guarded(T, E, BF, E + 8)
    lse = guarded(1, Bt * Hh * N, F32)
    ok(lib, lib.pevit_op_attn_fwd(S(), P(c["q"]), P(c["k"]), P(c["v"]), P(out), E + 8, P(lse), Bt, Hh, N))
    ok(lib, lib.pevit_op_attn_fwd(S(), P(c["q"]), P(c["k"]), P(c["v"]), P(out_inf), E + 8, None, Bt, Hh, N))
    assert guard_intact(out, T, E) and guard_intact(out_inf, T, E) and guard_intact(lse, 1, Bt * Hh * N)
    assert finite(out[:T, :E], lse[0]), "NaN or inf in out / lse"
    assert same_bits(out_inf, out)
    return out, lse


@pytest.mark.parametrize("N", H.ATTN_N)
@pytest.mark.parametrize("regime", H.ATTN_REGIMES)
def test_attention_core(lib, regime, N):
    Bt, Hh = H.ATTN_BT, H.ATTN_H
    E, T, ld = Hh * 64, Bt * N, 3 * Hh * 64 + 64
    c = attn_gpu(regime, N)
    out, lse = attn_fwd(lib, c, Bt, Hh, N)
    do = torch.full((T + 1, E + 16), NAN, dtype=BF, device="cuda")
    do[:T, :E] = c["do"]
    dqkv = guarded(T, 3 * E, BF, ld)
    ok(lib, lib.pevit_op_attn_bwd(S(), P(c["q"]), P(c["k"]), P(c["v"]), P(out), E + 8, P(do), E + 16, P(lse), P(dqkv), ld, Bt, Hh, N))
    assert guard_intact(dqkv, T, 3 * E) and finite(dqkv[:T, :3 * E]), "NaN or inf in dqkv"
    got = [heads_of(out[:T, :E].contiguous(), Bt, Hh, N).cpu(), lse[0].view(Bt * Hh, N).cpu()] + \
        [heads_of(dqkv[:T, i * E:(i + 1) * E].contiguous(), Bt, Hh, N).cpu() for i in range(3)]
    fig = H.attn_figures(got, c["ref"], regime)
    say(f"attn {regime} N={N}", fig, {n: H.attn_gate(regime, N, n) for n in fig})
    if regime == "onehot":                       # out IS v[h(i)]
        assert same_bits(got[0], c["v"][:, H.hot_key(N)].cpu())


@pytest.mark.parametrize("N", H.ATTN_N)
@pytest.mark.parametrize("regime", H.ATTN_REGIMES)
def test_attention_probs(lib, regime, N):
    """exp(q k^T - lse) with the exact lse and with the lse the forward kernel stored: finite, rows sum to 1"""
    Bt, Hh = H.ATTN_BT, H.ATTN_H
    c = attn_gpu(regime, N)
    _, lse_k = attn_fwd(lib, c, Bt, Hh, N)
    fig, gates = {}, {}
    for name, lse, tol in (("rowsum_exact", c["ref"][1].float().reshape(-1).cuda(), H.ROWSUM_EXACT_TOL),
                           ("rowsum_kernel", lse_k[0].contiguous(), H.ROWSUM_BF16_LSE_TOL)):
        for average in (0, 1):
            n = Bt * N * N * (1 if average else Hh)
            buf = guarded(1, n, F32)
            ok(lib, lib.pevit_op_attn_probs(S(), P(c["q"]), P(c["k"]), P(lse), P(buf), Bt, Hh, N, average))
            assert guard_intact(buf, 1, n) and finite(buf[0]), "NaN or inf in the probabilities"
            p = buf[0].view(-1, N).double()
            assert float(p.min()) >= 0
            key = f"{name}/{'mean' if average else 'heads'}"
            fig[key] = float((p.sum(-1) - 1).abs().max())
            gates[key] = H.gate_of(("attn", regime, N, name), tol)
    say(f"probs {regime} N={N}", fig, gates)


@pytest.mark.parametrize("N", H.CAUSAL_N)
@pytest.mark.parametrize("regime", H.CAUSAL_REGIMES)
def test_causal_attention(lib, regime, N):
    Bt, Hh = H.ATTN_BT, H.ATTN_H
    E, T = Hh * 64, Bt * N
    q, k, v, _ = H.attn_inputs(regime, N, causal=True)
    ref = H.causal_fwd(q, k, v)
    out = guarded(T, E, BF, E + 8)
    gq, gk, gv = q.cuda(), k.cuda(), v.cuda()
    ok(lib, lib.pevit_op_attn_fwd_causal(S(), P(gq), P(gk), P(gv), P(out), E + 8, Bt, Hh, N))
    assert guard_intact(out, T, E) and finite(out[:T, :E])
    got = heads_of(out[:T, :E].contiguous(), Bt, Hh, N).cpu()
    say(f"causal {regime} N={N}", {"out": max_rel(got.float(), ref)}, {"out": H.gate_of(("causal", regime, N, "out"), H.OUT_GATE)})
    assert same_bits(got[:, 0], v[:, 0]), "row 0 sees key 0 only"
    if regime == "onehot":
        assert same_bits(got, v[:, H.hot_key(N, True)])


@pytest.mark.parametrize("regime", ["peaked4", "offset"])
def test_fused_delta_attention(lib, regime):
    """pevit_op_attn_fwd_delta at a six-head geometry with a zero delta (t = 0, no bias): q and v come back unchanged and the
    attention core is the float64 one"""
    Bt, Hh, N = H.DELTA_GEOMETRY
    E, T = Hh * 64, Bt * N
    assert lib.pevit_op_attn_delta_hpw(Bt, Hh, N) > 0
    c = attn_gpu(regime, N, Bt, Hh)
    q, k, v = c["q"].clone(), c["k"].clone(), c["v"].clone()
    t = torch.zeros((T, 64), device="cuda")
    q16 = (torch.randn(E, 64, generator=torch.Generator().manual_seed(5)) * 0.1).to(BF).cuda()
    out, out_inf, lse = guarded(T, E, BF), guarded(T, E, BF), guarded(1, Bt * Hh * N, F32)
    ok(lib, lib.pevit_op_attn_fwd_delta(S(), P(q), P(k), P(v), P(t), P(q16), None, 160.0, P(out), E, P(lse), Bt, Hh, N))
    ok(lib, lib.pevit_op_attn_fwd_delta(S(), P(q), P(k), P(v), P(t), P(q16), None, 160.0, P(out_inf), E, None, Bt, Hh, N))
    assert guard_intact(out, T, E) and guard_intact(lse, 1, Bt * Hh * N) and finite(out[:T], lse[0])
    assert same_bits(q, c["q"]) and same_bits(k, c["k"]) and same_bits(v, c["v"]) and same_bits(out_inf, out)
    fig = {"out": max_rel(heads_of(out[:T], Bt, Hh, N).cpu().float(), c["ref"][0]),
           "lse": float((lse[0].view(Bt * Hh, N).cpu().double() - c["ref"][1]).abs().max())}
    say(f"delta {regime}", fig, {"out": H.OUT_GATE, "lse": H.LSE_GATE})
    plain, lse2 = attn_fwd(lib, c, Bt, Hh, N)
    assert same_bits(plain[:T, :E].contiguous(), out[:T]) and same_bits(lse2, lse)


# ======================================================================================================== 2. LayerNorm
@pytest.mark.parametrize("E", H.LN_WIDTHS)
@pytest.mark.parametrize("regime", H.LN_REGIMES)
def test_layernorm(lib, regime, E):
    """ln_fwd, then ln_bwd, the bf16-stream form of ln_bwd_ex and ln_bwd_affine on the mean / rstd that the forward launch stored"""
    rows = H.LN_ROWS
    c = H.ln_inputs(regime, E)
    g = {k: v.cuda() for k, v in c.items()}
    yb, yf = guarded(rows, E, BF), guarded(rows, E, F32)
    mean, rstd = guarded(1, rows, F32), guarded(1, rows, F32)
    ok(lib, lib.pevit_op_ln_fwd(S(), P(g["x"]), P(g["g"]), P(g["b"]), rows, E, P(yb), P(yf), P(mean), P(rstd)))
    assert guard_intact(yb, rows, E) and guard_intact(yf, rows, E) and guard_intact(mean, 1, rows) and guard_intact(rstd, 1, rows)
    dx, dxb = guarded(rows, E, F32), guarded(rows, E, BF)
    ok(lib, lib.pevit_op_ln_bwd(S(), P(g["dy"]), P(g["x"]), P(mean), P(rstd), P(g["g"]), P(g["dres"]), P(dx), P(dxb), rows, E))
    assert guard_intact(dx, rows, E) and guard_intact(dxb, rows, E)
    got = dict(y=yf[:rows], y16=yb[:rows], mean=mean[0], rstd=rstd[0], dx=dx[:rows], dx16=dxb[:rows])
    # the bf16 gradient stream: dy and the residual gradient in bf16
    ex, exb = guarded(rows, E, F32), guarded(rows, E, BF)
    ok(lib, lib.pevit_op_ln_bwd_ex(S(), P(g["dy16"]), 1, P(g["x"]), P(mean), P(rstd), P(g["g"]), P(g["dres16"]), 1, 0, P(ex), P(exb),
                                   rows, E, 0, None, None))
    assert guard_intact(ex, rows, E) and guard_intact(exb, rows, E)
    # the affine form: the same dx and the column sums of d gamma, d beta, d b_up
    blocks = lib.pevit_op_lna_blocks(rows)
    partial = guarded(blocks, 3 * E, F32)
    ax, axb = guarded(rows, E, F32), guarded(rows, E, BF)
    ok(lib, lib.pevit_op_ln_bwd_affine(S(), P(g["dy"]), P(g["x"]), P(mean), P(rstd), P(g["g"]), P(g["dres"]), P(ax), P(axb), P(partial),
                                       rows, E))
    assert guard_intact(partial, blocks, 3 * E) and guard_intact(ax, rows, E) and guard_intact(axb, rows, E)
    sums = partial[:blocks].view(blocks, 3, E).double().sum(0)
    got.update(dgamma=sums[0], dbeta=sums[1], dresum=sums[2])
    assert finite(*got.values(), ex[:rows], exb[:rows], ax[:rows], axb[:rows]), "NaN or inf"
    got = {k: v.cpu() for k, v in got.items()}
    ref = H.ln_ref(c)
    fig = H.ln_figures(got, ref)
    ref16 = H.ln_ref(c, c["dy16"], c["dres16"])
    fig["dx/bf16 stream"], fig["dx16/bf16 stream"] = max_rel(ex[:rows].cpu(), ref16["dx"]), max_rel(exb[:rows].cpu().float(), ref16["dx"])
    fig["dx/affine"], fig["dx16/affine"] = max_rel(ax[:rows].cpu(), ref["dx"]), max_rel(axb[:rows].cpu().float(), ref["dx"])
    say(f"ln {regime} E={E}", fig, {k: H.ln_gate(regime, E, k.split("/")[0]) for k in fig})
    if regime == "constant":
        assert same_bits(got["y"], c["b"].expand(rows, E).contiguous()), "y != beta on constant rows"
        assert torch.equal(got["mean"], c["x"][:, 0])
        assert float((got["rstd"].double() - H.RSTD_CONST).abs().max()) <= 2 * 2.0 ** -15


def test_fused_adapter_layernorm(lib):
    """the LayerNorm inside adapter_fwd_kernel (E = 768, T = 37): the rows h = hraw + bpr are the regimes' rows"""
    from test_adapter_fused_host import case as adapter_case, on
    from test_gpu_adapter_fused import fwd_payload, launch_fwd
    E, T = 768, H.LN_ROWS
    for regime in H.LN_REGIMES:
        c = H.ln_inputs(regime, E)
        a = dict(adapter_case(E, T))
        off = {"eps_offset": 0.5, "offset64": 64.0, "offset1024": 1024.0}.get(regime, 0.0)
        a["bpr"] = torch.full((E,), off)
        a["hraw"] = c["x"] - off
        h = a["hraw"] + a["bpr"]                       # what the kernel normalises (f32 sum of the two)
        a["gamma"], a["beta"] = c["g"], c["b"]
        got = fwd_payload(launch_fwd(lib, on(a, "cuda"), 0), T, 0)
        ref = H.ln_ref(dict(c, x=h))
        fig = {"z": max_rel(got["z"].cpu().float(), ref["y"]), "mean": max_rel(got["mean_a"].cpu(), ref["mean"]),
               "rstd": max_rel(got["rstd_a"].cpu(), ref["rstd"])}
        say(f"adapter ln {regime}", fig, {"z": H.ln_gate(regime, E, "y16"), "mean": H.ln_gate(regime, E, "mean"),
                                          "rstd": H.ln_gate(regime, E, "rstd")})
        if regime == "constant":
            assert same_bits(got["z"].cpu(), c["b"].to(BF).expand(T, E).contiguous()) and torch.equal(got["mean_a"].cpu(), h[:, 0])


# ======================================================================================================== 3. + 4. the head
def head_launch(lib, c, training, form="full"):
    from test_gpu_head import launch
    return launch(lib, c, training, form=form)


@pytest.mark.parametrize("regime", H.BN_REGIMES)
def test_head_batchnorm(lib, regime):
    from test_head_host import head_ref
    c, training = H.bn_case(regime), H.BN_TRAINING[regime]
    out = head_launch(lib, c, training)
    assert finite(*out.values())
    fig = H.head_figures({k: out[k] for k in H.BN_KEYS}, head_ref(c, training), H.BN_KEYS)
    say(f"head bn {regime}", fig, {k: H.head_gate("bn", regime, k) for k in fig})
    if not training:
        assert same_bits(out["rm"], c["rm0"]) and same_bits(out["rv"], c["rv0"])
    if regime == "const_col":                    # a constant column: ybn is exactly 0 and rstd = 1 / sqrt(eps)
        for col in (0, 5, c["D"] - 1):
            assert float(out["ybn"][:, col].abs().max()) == 0.0
            assert abs(float(out["rstd"][col]) - H.RSTD_CONST) <= 2 * 2.0 ** -15


def check_loss(tag, out, c, section, shape):
    assert torch.equal(out["logits"], c["want_logits"]), "the head's logits are not the stated ones"
    ref = H.loss_ref(c)
    assert finite(out["dlogits"], out["loss"])
    fig = H.head_figures(out, ref, ("dlogits",))
    say(tag, fig, {k: H.head_gate(section, shape, k) for k in fig})


@pytest.mark.parametrize("B,D,Cc", H.LOSS_SHAPES)
def test_head_cross_entropy_at_extreme_logits(lib, B, D, Cc):
    c = H.ce_case(B, D, Cc)
    out = head_launch(lib, c, False)
    assert bool((out["rstd"] == 1).all())
    check_loss(f"ce ({B},{D},{Cc})", out, c, "ce", (B, D, Cc))
    rl = head_launch(lib, c, False, form="no_dfeat")
    assert same_bits(rl["dlogits"], out["dlogits"]) and same_bits(rl["loss"], out["loss"])
    check_loss(f"ce row losses ({B},{D},{Cc})", rl, c, "ce", (B, D, Cc))


@pytest.mark.parametrize("B,D,Cc", H.LOSS_SHAPES)
def test_head_bce_at_extreme_logits(lib, B, D, Cc):
    c = H.bce_case(B, D, Cc)
    out = head_launch(lib, c, False)
    check_loss(f"bce ({B},{D},{Cc})", out, c, "bce", (B, D, Cc))


@pytest.mark.parametrize("B,D,Cc", [H.LOSS_SHAPES[0], H.LOSS_SHAPES[2]])
def test_head_all_rows_ignored(lib, B, D, Cc):
    """what F.cross_entropy returns for a batch of ignore_index rows (test_all_rows_ignored_is_what_torch_returns): a NaN loss,
    the mean over zero rows, and a zero gradient"""
    c = H.ce_case(B, D, Cc, all_ignored=True)
    out = head_launch(lib, c, False, form="no_dfeat")
    assert torch.equal(out["logits"], c["want_logits"])
    assert bool(torch.isnan(out["loss"])) and float(out["dlogits"].abs().max()) == 0.0 and float(out["rowloss"].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the probe's own head and losses
def probe_run(c, training):
    """one pevit_probe_step (no update) on the case's rows, gathered through a reversed index: logits, loss, dW, db, running stats"""
    from test_gpu_probe import _engine
    B, D, Cc = c["B"], c["D"], c["C"]
    eng = _engine(D, Cc, max_batch=64)          # (an engine of its own: the key differs from test_gpu_probe's)
    v = eng.param_views()
    with torch.no_grad():
        v["layers.0.weight"].copy_(c["W"].cuda()); v["layers.0.bias"].copy_(c["bias"].cuda())
        eng.running_mean.copy_(c["rm0"].cuda()); eng.running_var.copy_(c["rv0"].cuda())
    eng.reset_optimizer()
    eng.grads.fill_(NAN)
    feats = c["feat"].flip(0).contiguous().cuda()
    idx = torch.arange(B - 1, -1, -1).cuda()
    labels = (c["labels"] if c["targets"] is None else c["targets"]).flip(0).contiguous().cuda()
    pred = eng.probe_predict(feats, index=idx)
    logits, loss = eng.probe_step(feats, idx, labels, bn_training=training, update=False)
    torch.cuda.synchronize()
    gv = eng.grad_views()
    return dict(pred=pred.cpu(), logits=logits.cpu(), loss=loss.cpu().reshape(()), gW=gv["layers.0.weight"].cpu().clone(),
                gb=gv["layers.0.bias"].cpu().clone(), rm=eng.running_mean.cpu().clone(), rv=eng.running_var.cpu().clone())


@pytest.mark.parametrize("regime", H.BN_REGIMES)
def test_probe_batchnorm(lib, regime):
    from test_head_host import head_ref
    c, training = H.bn_case(regime), H.BN_TRAINING[regime]
    out = probe_run(c, training)
    assert finite(*out.values())
    r = dict(head_ref(c, training))
    r["gW"], r["gb"] = r["gW"] - c["gW0"].double(), r["gb"] - c["gb0"].double()          # the probe writes its gradients
    fig = H.head_figures({k: out[k] for k in ("logits", "gW", "gb", "rm", "rv")}, r, ("logits", "gW", "gb", "rm", "rv"))
    if not training:
        fig["predict"] = max_rel(out["pred"], r["logits"])
        assert same_bits(out["rm"], c["rm0"]) and same_bits(out["rv"], c["rv0"])
    say(f"probe bn {regime}", fig, {k: H.head_gate("bn", regime, "logits" if k == "predict" else k) for k in fig})


@pytest.mark.parametrize("kind", ["ce", "bce"])
@pytest.mark.parametrize("B,D,Cc", H.LOSS_SHAPES[:2])
def test_probe_losses_at_extreme_logits(lib, B, D, Cc, kind):
    c = H.ce_case(B, D, Cc) if kind == "ce" else H.bce_case(B, D, Cc)
    out = probe_run(c, False)
    assert torch.equal(out["logits"], c["want_logits"]) and torch.equal(out["pred"], c["want_logits"])
    assert finite(out["loss"], out["gW"], out["gb"])
    ref = H.loss_ref(c)
    want = dict(loss=ref["loss"], gW=ref["dlogits"].T @ c["feat"].double(), gb=ref["dlogits"].sum(0))
    fig = H.head_figures(out, want, ("gW", "gb"))
    say(f"probe {kind} ({B},{D},{Cc})", fig, {k: H.head_gate(kind, (B, D, Cc), k) for k in fig})


def test_probe_all_rows_ignored(lib):
    c = H.ce_case(*H.LOSS_SHAPES[0], all_ignored=True)
    out = probe_run(c, False)
    assert bool(torch.isnan(out["loss"])) and float(out["gW"].abs().max()) == 0.0 and float(out["gb"].abs().max()) == 0.0


# ======================================================================================================== 5. GELU epilogues
GEMM_M, GEMM_N, GEMM_K = 128, 128, 64
EPI = dict(quick=2, dquick=3, new=10, dnew=12, drelu=11)       # BIAS_GELU, DGELU, BIAS_GELUNEW, DGELUNEW, DRELU (csrc/kernels.h)


def grid_columns(n):
    g = H.gelu_grid()
    return g[torch.arange(n) % g.numel()]


def gemm_epilogue(lib, kind):
    """one pevit_op_gemm_ex whose accumulator is exactly 0 (forward: the pre-activation is the bias) or exactly 1 (derivatives: the
    result is f'(aux)); returns the pre-activations per column and the [M][N] bf16 result"""
    from pevit_amd._lib import PevitGemmExArgs
    M, N, K = GEMM_M, GEMM_N, GEMM_K
    x = grid_columns(N)
    deriv = kind in ("dquick", "dnew", "drelu")
    A = torch.zeros((M + 8, K), dtype=BF, device="cuda")
    B = (torch.randn(N + 8, K, generator=torch.Generator().manual_seed(3))).to(BF).cuda()
    if deriv:
        A[:M, 0] = 1.0
        B.zero_()
        B[:N, 0] = 1.0
    bias = (torch.zeros(N) if deriv else x.clone()).cuda()
    aux = x.to(BF).expand(M + 8, N).contiguous().cuda()
    outb, outb2 = guarded(M, N, BF, N + 8), guarded(M, N, BF, N + 8)
    a = PevitGemmExArgs()
    a.epilogue, a.M, a.N, a.K = EPI[kind], M, N, K
    a.A, a.lda, a.B, a.ldb, a.b_rows = A.data_ptr(), K, B.data_ptr(), K, N + 8
    a.bias = bias.data_ptr()
    a.out_bf16, a.ldob = outb.data_ptr(), N + 8
    if deriv:
        a.aux_bf16, a.ldaux = aux.data_ptr(), N
    else:
        a.out2_bf16, a.ldob2 = outb2.data_ptr(), N + 8
    ok(lib, lib.pevit_op_gemm_ex(S(), C.byref(a)))
    assert guard_intact(outb, M, N) and (deriv or guard_intact(outb2, M, N))
    if not deriv:                                # the stored pre-activation is the bias, exactly (0 + -0 = +0: the sign of a zero goes)
        h = outb[:M, :N].contiguous().cpu()
        assert torch.equal(h.float(), x.expand(M, N)) and same_bits(h[:, x != 0], x.to(BF).expand(M, N)[:, x != 0])
        x = h[0].float()
    return x, (outb if deriv else outb2)[:M, :N].contiguous().cpu()


@pytest.mark.parametrize("kind", H.GELU_KINDS)
def test_gemm_gelu_epilogues(lib, kind):
    x, got = gemm_epilogue(lib, kind)
    f = H.gelu_check(kind, got, x.expand(GEMM_M, GEMM_N))
    print(f"\ngemm {kind}: largest relative deviation {f:.2e} (gate {H.GELU_GATE})", end="")


def test_gemm_drelu_at_signed_zeros(lib):
    x, got = gemm_epilogue(lib, "drelu")
    want = (x > 0).to(BF).expand(GEMM_M, GEMM_N).contiguous()          # aux = +-0: exactly +0
    assert same_bits(got, want)


def test_fused_adapter_gelu_new(lib):
    """the gelu_new path of the fused adapter kernels: W_down = 0 puts the pre-activation on b_down (forward); dyb W_up^T = 1 and
    the saved pre-activation on the grid give gelu_new' itself (backward)"""
    from test_adapter_fused_host import case as adapter_case, on
    from test_gpu_adapter_fused import bwd_payload, fwd_payload, launch_bwd, launch_fwd
    E, T = 768, H.LN_ROWS
    x = grid_columns(64)
    a = dict(adapter_case(E, T))
    a["wd"] = torch.zeros_like(a["wd"])
    a["b_down"] = x.clone()
    got = fwd_payload(launch_fwd(lib, on(a, "cuda"), 1), T, 1)
    apre = got["apre"].cpu()                      # 0 + -0 = +0: the sign of a zero goes, everything else is b_down to the bit
    assert torch.equal(apre.float(), x.expand(T, 64)) and same_bits(apre[:, x != 0], x.to(BF).expand(T, 64)[:, x != 0])
    f = H.gelu_check("new", got["act"].cpu(), apre.float())
    print(f"\nadapter gelu_new: largest relative deviation {f:.2e}", end="")
    b = dict(adapter_case(E, T))
    b["dyb"] = torch.zeros(T, E, dtype=BF)
    b["dyb"][:, 0] = 1.0
    b["wuT"] = torch.zeros(64, E, dtype=BF)
    b["wuT"][:, 0] = 1.0
    b["wdT"] = torch.zeros_like(b["wdT"])
    g = on(b, "cuda")
    saved = x.to(BF).expand(T, 64).contiguous().cuda()
    mean_a, rstd_a = torch.zeros(T, device="cuda"), torch.ones(T, device="cuda")
    rc, buf, nb = launch_bwd(lib, g, 1, (saved, mean_a, rstd_a), None)
    ok(lib, rc)
    out = bwd_payload(buf, T, E, nb)
    f = H.gelu_check("dnew", out["dpre"].cpu(), x.expand(T, 64))
    print(f"  gelu_new': {f:.2e}", end="")


# ======================================================================================================== 6. fp8 row scales
def test_fp8_row_scales_at_their_boundaries(lib):
    from pevit_amd import fp8
    rows, cols = H.FP8_SHAPE
    w, _ = H.fp8_rows()
    gw = w.cuda()
    codes = torch.full((256, cols), 0x7F, dtype=torch.uint8, device="cuda")
    scales = guarded(1, rows, F32)
    ok(lib, lib.pevit_op_quant_fp8(S(), P(gw), rows, cols, P(codes), P(scales), None))
    assert guard_intact(scales, 1, rows) and bool((codes[rows:] == 0x7F).all())
    ref_codes, ref_scales = fp8.quantize_rows(w)
    assert torch.equal(scales[0].cpu(), ref_scales)
    got = torch.empty_like(ref_codes)
    got[:, torch.arange(cols)] = codes[:rows].cpu()[:, fp8.kperm(cols)]
    assert not bool(((got & 0x7F) == 0x7F).any()), "a code is the NaN pattern"
    a, b = got.view(torch.float8_e4m3fn).float(), ref_codes.view(torch.float8_e4m3fn).float()
    assert torch.equal(a, b) and torch.equal(got[b != 0], ref_codes[b != 0])
    out = guarded(rows, cols, F32)
    ok(lib, lib.pevit_op_dequant_fp8(S(), P(codes), P(scales), rows, cols, P(out)))
    assert guard_intact(out, rows, cols) and torch.equal(out[:rows].cpu(), fp8.dequantize_rows(ref_codes, ref_scales))
