"""The attention and LayerNorm kernel forms that tests/test_gpu_ops.py does not launch, one kernel at a time through the C ABI.

1. Token-count sweep of attn_fwd / attn_bwd / attn_probs (the plain pevit_op_* entry points) over
   N in {65, 128, 129, 144, 145, 224, 225, 226, 272, 273, 288}: the two runtime-N forward instances, the backward kernel's shared
   last tile (N in [129, 144] on 8 waves, [257, 272] on 16), the family boundaries 64|65 and 224|225 and the cap 288, with row
   pitches that are NOT the width (ldo = E + 8, lddo = E + 16, ld = 3E + 64).  Which instance an N lands in follows from N alone
   (the table is in tests/test_kernel_forms_host.py), so no launch-path introspection is needed or used.  Reference: float64 torch
   on the same bf16 operands; gates: the ones of test_gpu_ops.py (out max-rel 1.5e-2, |lse - ref| 2e-2, gradients rel-L2 2e-2) and
   of test_gpu_attention_seam.py (probabilities 1e-5 absolute, row sums 1e-5 / 2.1e-3).  The last token's k, v and dO rows are
   doubled so that those whole-tensor gates see an off-by-one key mask; tests/test_kernel_forms_host.py proves that on the CPU and
   prints the rounding floor of a bf16 emulation of the kernels against float64, over the eleven N:
       out max-rel 2.0e-3 .. 2.9e-3    lse 1.0e-3 .. 1.4e-3    dQ 3.6e-3 .. 4.8e-3    dK 3.1e-3 .. 3.7e-3    dV 2.2e-3 .. 2.4e-3
   (last key counted twice: out >= 1.7e-1, lse 6.9e-1, dQ >= 2.0e-1, dK >= 1.3e-1, dV >= 8.2e-2; dropped: everything >= 4.2e-1).
   The kernels land on that floor: on the MI355X the sweep measured out 2.0e-3 .. 2.9e-3, lse 1.0e-3 .. 1.4e-3, dQ 3.6e-3 .. 4.8e-3,
   dK 3.1e-3 .. 3.7e-3, dV 2.2e-3 .. 2.4e-3, within a few per cent of the emulation's figure at every N.

2. The forms that only the training step selects, through the test-only pevit_op_*_ex entry points (csrc/verify.hip: they fill
   the launchers' parameter structs and add no kernel):
     * LayerNorm backward with bf16 dy and the bf16 residual gradient (separate, in place, in place without the f32 output), the
       class-token residual period, the class-token row stride and both power-of-two column scales, for every width instance
       (generic with partly masked column groups: 128, 320, 1000; NV = 1..4: 256, 512, 768, 1024) -- held to a float64 LayerNorm
       backward of the stored operands at the gates of test_layernorm_fwd_bwd (f32 2e-5, bf16 1e-2) and to identities that are
       exact by construction (one f32 value feeds both stores; the scales are powers of two);
     * LayerNorm forward with the class-token row stride and the e4m3 copy;
     * the attention forward's e4m3 copy and the attention backward's class-token-only dO.

Every output buffer is pre-filled with NaN (an unwritten element fails) and carries pad columns / a guard row holding a sentinel
that must survive; operands that a form promises not to read hold NaN.
"""
import ctypes as C
import functools

import pytest
import torch

from conftest import max_rel, rel_err
from test_kernel_forms_host import (GRAD_GATE, LSE_GATE, OUT_GATE, SWEEP_BT, SWEEP_H, SWEEP_N, attn_ref64, heads_of, rows_of,
                                    sweep_inputs)

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -7.0                      # sentinel of pad columns and guard rows (exact in bf16)
PROBS_TOL, ROWSUM_EXACT_TOL, ROWSUM_BF16_LSE_TOL = 1e-5, 1e-5, 2.1e-3      # tests/test_gpu_attention_seam.py


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
    torch.cuda.synchronize()


def refused(lib, rc, *words):
    assert rc == -1
    msg = lib.pevit_last_error().decode()
    for w in words:
        assert w in msg, msg


def rnd(*shape, scale=1.0, seed=0, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def bits(t):
    """bf16 / f32 / u8 tensor as integers: NaN-safe, sign-of-zero-strict equality"""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def guarded(rows, width, dtype, pitch=None, fill=NAN):
    """[rows + 1][pitch] buffer: the payload [rows][width] holds `fill`, the pad columns and the guard row the sentinel"""
    t = torch.full((rows + 1, pitch or width), SENT, dtype=dtype, device="cuda")
    t[:rows, :width] = fill
    return t


def guard_intact(t, rows, width):
    return bool((t[rows:] == SENT).all()) and bool((t[:rows, width:] == SENT).all())


# ------------------------------------------------------------------------------------------------ 1. the token-count sweep
@functools.lru_cache(maxsize=None)
def sweep_case(N):
    """inputs on the GPU and the float64 reference (computed once per N, shared by the sweep tests, never modified)"""
    Bt, H = SWEEP_BT, SWEEP_H
    q, k, v, do = (t.cuda() for t in sweep_inputs(N))
    out, lse, dq, dk, dv = attn_ref64(q, k, v, heads_of(do, Bt, H, N))
    s64 = torch.bmm(q.double(), k.double().transpose(1, 2))
    return dict(q=q, k=k, v=v, do=do, out=rows_of(out, Bt, H, N), lse=lse, s64=s64,
                grads=[rows_of(g, Bt, H, N) for g in (dq, dk, dv)])


@pytest.mark.parametrize("N", SWEEP_N)
def test_attention_token_count_sweep(lib, N):
    Bt, H = SWEEP_BT, SWEEP_H
    E, T = H * 64, Bt * N
    ldo, lddo, ld = E + 8, E + 16, 3 * E + 64
    c = sweep_case(N)
    q, k, v = c["q"], c["k"], c["v"]
    out = guarded(T, E, torch.bfloat16, ldo)
    lse = guarded(1, Bt * H * N, torch.float32)
    ok(lib, lib.pevit_op_attn_fwd(S(), P(q), P(k), P(v), P(out), ldo, P(lse), Bt, H, N))
    out_inf = guarded(T, E, torch.bfloat16, ldo)
    ok(lib, lib.pevit_op_attn_fwd(S(), P(q), P(k), P(v), P(out_inf), ldo, None, Bt, H, N))      # the instance without the lse store
    assert guard_intact(out, T, E) and guard_intact(out_inf, T, E) and guard_intact(lse, 1, Bt * H * N)
    assert torch.isfinite(out[:T, :E].float()).all() and torch.isfinite(lse[0]).all()
    assert same_bits(out_inf, out)
    e_out = max_rel(out[:T, :E].float(), c["out"])
    e_lse = float((lse[0].view(Bt * H, N).double() - c["lse"]).abs().max())
    print(f"\nN={N}: out max-rel {e_out:.3e}  lse max-abs {e_lse:.3e}", end="")
    assert e_out < OUT_GATE
    assert e_lse < LSE_GATE

    # the pad columns and the guard row of dO hold NaN: they are not read
    do = torch.full((T + 1, lddo), NAN, dtype=torch.bfloat16, device="cuda")
    do[:T, :E] = c["do"]
    dqkv = guarded(T, 3 * E, torch.bfloat16, ld)
    ok(lib, lib.pevit_op_attn_bwd(S(), P(q), P(k), P(v), P(out), ldo, P(do), lddo, P(lse), P(dqkv), ld, Bt, H, N))
    assert guard_intact(dqkv, T, 3 * E)                         # the u columns [3E, ld) and the row behind the last are not touched
    assert torch.isfinite(dqkv[:T, :3 * E].float()).all()
    errs = [rel_err(dqkv[:T, i * E:(i + 1) * E].float(), g) for i, g in enumerate(c["grads"])]
    print("  dq %.3e  dk %.3e  dv %.3e (rel-L2)" % tuple(errs))
    for i, e in enumerate(errs):
        assert e < GRAD_GATE, ("dq dk dv".split()[i], e)


def _check_probs(lib, q, k, s64, lse, rowsum_tol, B, H, N):
    mean = guarded(1, B * N * N, torch.float32)
    heads = guarded(1, B * H * N * N, torch.float32)
    ok(lib, lib.pevit_op_attn_probs(S(), P(q), P(k), P(lse), P(mean), B, H, N, 1))
    ok(lib, lib.pevit_op_attn_probs(S(), P(q), P(k), P(lse), P(heads), B, H, N, 0))
    assert guard_intact(mean, 1, B * N * N) and guard_intact(heads, 1, B * H * N * N)
    ref = torch.exp(s64 - lse.double().view(B * H, N, 1)).view(B, H, N, N)
    for name, got, want in (("heads", heads[0].view(B, H, N, N), ref), ("mean", mean[0].view(B, N, N), ref.sum(1) / H)):
        got = got.double()
        assert torch.isfinite(got).all()
        e_sum, e_abs = float((got.sum(-1) - 1).abs().max()), float((got - want).abs().max())
        print(f"\nN={N} {name}: row sums off by {e_sum:.3e} (gate {rowsum_tol:.1e}), max-abs {e_abs:.3e}", end="")
        assert e_sum < rowsum_tol
        assert e_abs < PROBS_TOL


@pytest.mark.parametrize("N", SWEEP_N)
def test_attention_probs_token_count_sweep(lib, N):
    """exp(q k^T - lse), per head and averaged: with the exact lse (rows sum to 1 within 1e-5) and with the lse the forward kernel
    saved (m + log of the bf16-rounded row sum: rows sum to 1 within 2.1e-3, tests/test_gpu_attention_seam.py)"""
    Bt, H = SWEEP_BT, SWEEP_H
    c = sweep_case(N)
    q, k, v, s64 = c["q"], c["k"], c["v"], c["s64"]
    out = torch.empty((Bt * N, H * 64), dtype=torch.bfloat16, device="cuda")
    lse_fwd = torch.full((Bt * H * N,), NAN, device="cuda")
    ok(lib, lib.pevit_op_attn_fwd(S(), P(q), P(k), P(v), P(out), H * 64, P(lse_fwd), Bt, H, N))
    lse_exact = torch.logsumexp(s64, dim=-1).float().reshape(-1).contiguous()
    _check_probs(lib, q, k, s64, lse_exact, ROWSUM_EXACT_TOL, Bt, H, N)
    _check_probs(lib, q, k, s64, lse_fwd, ROWSUM_BF16_LSE_TOL, Bt, H, N)


def test_attention_probs_beyond_the_core_limit(lib):
    """attn_probs alone takes N up to 384 (twelve 32-key blocks: its three-blocks-per-wave instance at its cap); lse from torch"""
    Bt, H, N = SWEEP_BT, SWEEP_H, 384
    q, k, _, _ = (t.cuda() for t in sweep_inputs(N))
    s64 = torch.bmm(q.double(), k.double().transpose(1, 2))
    lse = torch.logsumexp(s64, dim=-1).float().reshape(-1).contiguous()
    _check_probs(lib, q, k, s64, lse, ROWSUM_EXACT_TOL, Bt, H, N)


@pytest.mark.parametrize("N", [0, 289])
def test_attention_refuses_token_counts_outside_its_range(lib, N):
    """argument checks before any launch"""
    H, E = 2, 128
    buf = torch.zeros((8, 3 * E + 64), dtype=torch.bfloat16, device="cuda")
    lse = torch.zeros(64, device="cuda")
    refused(lib, lib.pevit_op_attn_fwd(S(), P(buf), P(buf), P(buf), P(buf), E, P(lse), 1, H, N), "attn_fwd", f"N={N}", "[1,288]")
    refused(lib, lib.pevit_op_attn_bwd(S(), P(buf), P(buf), P(buf), P(buf), E, P(buf), E, P(lse), P(buf), 3 * E + 64, 1, H, N),
            "attn_bwd", f"N={N}", "[1,288]")
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 2a. LayerNorm backward
LN_BT, LN_N = 3, 10
LN_ROWS = LN_BT * LN_N                 # 30 rows: 7 whole workgroups of 4 rows and a partial one
LN_WIDTHS = [128, 320, 1000, 256, 512, 768, 1024]      # generic instance (masked column groups) x 3, NV = 1 .. 4
ln_forms = pytest.mark.parametrize("scaled", [False, True], ids=["plain", "colscales"])
ln_widths = pytest.mark.parametrize("E", LN_WIDTHS)


def pow2(n, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.ldexp(torch.ones(n), torch.randint(-6, 7, (n,), generator=g)).cuda()


@functools.lru_cache(maxsize=None)
def ln_case(E):
    """operands (never modified) and the float64 LayerNorm backward of the STORED operands, without the residual gradient"""
    from pevit_amd import _lib
    lib = _lib.load()
    rows = LN_ROWS
    x = rnd(rows, E, seed=1, scale=2.0) + 0.5
    g = 1 + rnd(E, seed=2, scale=0.2); b = rnd(E, seed=3, scale=0.2)
    mean = torch.full((rows,), NAN, device="cuda"); rstd = torch.full((rows,), NAN, device="cuda")
    yf = torch.empty((rows, E), device="cuda")
    ok(lib, lib.pevit_op_ln_fwd(S(), P(x), P(g), P(b), rows, E, None, P(yf), P(mean), P(rstd)))
    dy = rnd(rows, E, seed=4, dtype=torch.bfloat16)            # bf16 in storage: what the dX GEMM hands over
    dres = rnd(rows, E, seed=5, dtype=torch.bfloat16)          # the bf16 gradient stream, values of order 1
    x64 = x.double()
    mu = x64.mean(-1, keepdim=True)
    r = torch.rsqrt(((x64 - mu) ** 2).mean(-1, keepdim=True) + 1e-5)
    xh = (x64 - mu) * r
    gd = dy.double() * g.double()
    ln64 = r * (gd - gd.mean(-1, keepdim=True) - xh * (gd * xh).mean(-1, keepdim=True))
    return dict(x=x, g=g, mean=mean, rstd=rstd, dy=dy, dres=dres, ln64=ln64, bs=pow2(E, 6), rs=pow2(E, 7))


def ln_bwd(lib, c, E, *, dy=None, x=None, mean=None, rstd=None, dres, dx, dxb, rows=LN_ROWS, res16=1, res_period=0, xstride=0,
           bs=None, rs=None):
    dy = c["dy"] if dy is None else dy
    return lib.pevit_op_ln_bwd_ex(S(), P(dy), int(dy.dtype == torch.bfloat16), P(c["x"] if x is None else x),
                                  P(c["mean"] if mean is None else mean), P(c["rstd"] if rstd is None else rstd), P(c["g"]),
                                  P(dres), res16, res_period, P(dx), P(dxb), rows, E, xstride, P(bs), P(rs))


def scales(c, scaled):
    return (c["bs"], c["rs"]) if scaled else (None, None)


@ln_widths
@ln_forms
def test_ln_bwd_bf16_stream_against_float64_and_in_place(lib, E, scaled):
    c, rows = ln_case(E), LN_ROWS
    bs, rs = scales(c, scaled)
    # the bf16 residual gradient in a buffer of its own, both outputs
    dx = guarded(rows, E, torch.float32); dxb = guarded(rows, E, torch.bfloat16)
    ok(lib, ln_bwd(lib, c, E, dres=c["dres"], dx=dx, dxb=dxb, bs=bs, rs=rs))
    assert guard_intact(dx, rows, E) and guard_intact(dxb, rows, E)
    want = c["ln64"] + c["dres"].double() / (rs.double() if scaled else 1.0)
    e32 = max_rel(dx[:rows], want)
    e16 = max_rel(dxb[:rows].float(), want * (bs.double() if scaled else 1.0))
    print(f"\nE={E} {'scaled' if scaled else 'plain'}: f32 max-rel {e32:.3e}  bf16 max-rel {e16:.3e}")
    assert e32 < 2e-5
    assert e16 < 1e-2
    # one f32 value feeds both stores; the column scales are powers of two
    assert same_bits(dxb[:rows], (dx[:rows] * bs if scaled else dx[:rows]).bfloat16())
    # ... read and rewritten in place (dres == dx_bf16), with and without the f32 output
    dx1 = guarded(rows, E, torch.float32); buf1 = guarded(rows, E, torch.bfloat16)
    buf1[:rows] = c["dres"]
    ok(lib, ln_bwd(lib, c, E, dres=buf1, dx=dx1, dxb=buf1, bs=bs, rs=rs))
    buf2 = guarded(rows, E, torch.bfloat16)
    buf2[:rows] = c["dres"]
    ok(lib, ln_bwd(lib, c, E, dres=buf2, dx=None, dxb=buf2, bs=bs, rs=rs))
    assert same_bits(dx1, dx) and same_bits(buf1, dxb) and same_bits(buf2, dxb)


@ln_widths
@ln_forms
def test_ln_bwd_residual_on_the_class_token_rows_only(lib, E, scaled):
    """res_period = N: the residual gradient exists on rows b*N only and nothing else of it is read (the other rows hold NaN) ==
    the full read of a residual gradient that is zero off those rows"""
    c, rows = ln_case(E), LN_ROWS
    bs, rs = scales(c, scaled)
    cls = torch.arange(rows, device="cuda") % LN_N == 0
    zeroed = torch.where(cls[:, None], c["dres"], torch.zeros_like(c["dres"]))
    holes = torch.where(cls[:, None], c["dres"], torch.full_like(c["dres"], NAN))
    dx0 = guarded(rows, E, torch.float32); b0 = guarded(rows, E, torch.bfloat16)
    ok(lib, ln_bwd(lib, c, E, dres=zeroed, dx=dx0, dxb=b0, bs=bs, rs=rs))
    want = c["ln64"] + zeroed.double() / (rs.double() if scaled else 1.0)
    assert max_rel(dx0[:rows], want) < 2e-5
    # the production form: in place on the bf16 stream, no f32 output
    buf = guarded(rows, E, torch.bfloat16)
    buf[:rows] = holes
    ok(lib, ln_bwd(lib, c, E, dres=buf, dx=None, dxb=buf, res_period=LN_N, bs=bs, rs=rs))
    assert same_bits(buf, b0)
    # and with a buffer of its own and the f32 output
    dx1 = guarded(rows, E, torch.float32); b1 = guarded(rows, E, torch.bfloat16)
    ok(lib, ln_bwd(lib, c, E, dres=holes, dx=dx1, dxb=b1, res_period=LN_N, bs=bs, rs=rs))
    assert same_bits(dx1, dx0) and same_bits(b1, b0)


@ln_widths
@ln_forms
def test_ln_bwd_class_token_row_stride(lib, E, scaled):
    """xstride = N*E, rows = Bt: x, the residual gradient and both outputs on the class-token rows of [Bt*N][E] buffers, dy / mean /
    rstd compact == the compact call on the gathered rows; the rows in between keep their sentinel"""
    c, Bt, N = ln_case(E), LN_BT, LN_N
    bs, rs = scales(c, scaled)
    dy = c["dy"][:Bt].contiguous()
    mean, rstd = c["mean"][::N].contiguous(), c["rstd"][::N].contiguous()
    # compact
    dx0 = guarded(Bt, E, torch.float32); b0 = guarded(Bt, E, torch.bfloat16)
    b0[:Bt] = c["dres"][::N]
    ok(lib, ln_bwd(lib, c, E, dy=dy, x=c["x"][::N].contiguous(), mean=mean, rstd=rstd, dres=b0, dx=dx0, dxb=b0, rows=Bt, bs=bs, rs=rs))
    assert torch.isfinite(dx0[:Bt]).all() and guard_intact(dx0, Bt, E) and guard_intact(b0, Bt, E)
    # strided, in place
    big32 = torch.full((Bt * N + 1, E), SENT, device="cuda"); big16 = torch.full((Bt * N + 1, E), SENT, dtype=torch.bfloat16, device="cuda")
    big16[:Bt * N:N] = c["dres"][::N]
    ok(lib, ln_bwd(lib, c, E, dy=dy, mean=mean, rstd=rstd, dres=big16, dx=big32, dxb=big16, rows=Bt, xstride=N * E, bs=bs, rs=rs))
    assert same_bits(big32[:Bt * N:N], dx0[:Bt]) and same_bits(big16[:Bt * N:N], b0[:Bt])
    off = torch.arange(Bt * N + 1, device="cuda") % N != 0
    off[Bt * N] = True                                         # the guard row
    assert bool((big32[off] == SENT).all()) and bool((big16[off] == SENT).all())


@ln_widths
def test_ln_bwd_residual_column_scales_are_taken_out_exactly(lib, E):
    """res_colscale == the call without it on a residual gradient divided by the (power-of-two) scales beforehand"""
    c, rows = ln_case(E), LN_ROWS
    out = []
    for dres, rs in ((c["dres"], c["rs"]), ((c["dres"].float() / c["rs"]).bfloat16(), None)):
        assert rs is not None or torch.equal(dres.float() * c["rs"], c["dres"].float())        # the division was exact
        dx = guarded(rows, E, torch.float32); dxb = guarded(rows, E, torch.bfloat16)
        ok(lib, ln_bwd(lib, c, E, dres=dres, dx=dx, dxb=dxb, bs=c["bs"], rs=rs))
        out.append((dx, dxb))
    assert torch.isfinite(out[0][0][:rows]).all()
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1])


def test_ln_bwd_bf16_residual_form_refusals(lib):
    E = 256
    c, rows = ln_case(E), LN_ROWS
    dx = guarded(rows, E, torch.float32); dxb = guarded(rows, E, torch.bfloat16)
    refused(lib, ln_bwd(lib, c, E, dy=c["dy"].float(), dres=c["dres"], dx=dx, dxb=dxb), "ln_bwd", "bf16 storage on both sides")
    refused(lib, ln_bwd(lib, c, E, dres=None, dx=dx, dxb=dxb), "ln_bwd", "dres (null)")
    torch.cuda.synchronize()
    assert torch.isnan(dx[:rows]).all() and torch.isnan(dxb[:rows].float()).all()       # nothing was launched


# ------------------------------------------------------------------------------------------------ 2b. LayerNorm forward
def ln_fwd(lib, x, g, b, rows, E, xstride, fp8=True):
    yb = guarded(rows, E, torch.bfloat16); yf = guarded(rows, E, torch.float32)
    mean = guarded(1, rows, torch.float32); rstd = guarded(1, rows, torch.float32)
    y8 = torch.full((rows + 1, E), 0x7F, dtype=torch.uint8, device="cuda") if fp8 else None      # 0x7F: the e4m3 NaN
    rc = lib.pevit_op_ln_fwd_ex(S(), P(x), P(g), P(b), rows, E, xstride, P(yb), P(yf), P(mean), P(rstd), P(y8))
    return rc, (yb, yf, mean, rstd, y8)


@pytest.mark.parametrize("E", [128, 768, 1024])
def test_ln_fwd_row_stride_and_fp8_copy(lib, E):
    from pevit_amd import fp8
    Bt, N = LN_BT, LN_N
    rows = Bt * N
    x = rnd(rows, E, seed=1, scale=2.0) + 0.5
    g = 1 + rnd(E, seed=2, scale=0.2); b = rnd(E, seed=3, scale=0.2)
    b[3], b[E - 5], b[E // 2 + 1] = 600.0, -700.0, 452.0          # outputs beyond +-448: the copy saturates
    # every row, compact: the e4m3 copy == cast_fp8 of the f32 output of the same launch
    rc, (yb, yf, mean, rstd, y8) = ln_fwd(lib, x, g, b, rows, E, 0)
    ok(lib, rc)
    assert guard_intact(yb, rows, E) and guard_intact(yf, rows, E) and guard_intact(mean, 1, rows) and bool((y8[rows] == 0x7F).all())
    ref = torch.nn.functional.layer_norm(x.double(), (E,), g.double(), b.double(), 1e-5)
    assert max_rel(yf[:rows], ref) < 1e-5 and max_rel(yb[:rows].float(), ref) < 1e-2
    assert float(yf[:rows].max()) > 448 and float(yf[:rows].min()) < -448
    codes = torch.full((rows, E), 0x7F, dtype=torch.uint8, device="cuda")
    ok(lib, lib.pevit_op_cast_fp8(S(), P(yf), P(codes), rows, E))
    assert same_bits(y8[:rows], codes)
    dec = y8[:rows].cpu()[:, fp8.kperm(E)].view(torch.float8_e4m3fn).float()          # channel c sits at position kperm(c)
    assert bool((dec[:, 3] == 448).all()) and bool((dec[:, E - 5] == -448).all())
    assert torch.equal(dec, yf[:rows].cpu().clamp(-448, 448).to(torch.float8_e4m3fn).float())
    # the class-token rows through the row stride == the compact call on the gathered rows
    rc, strided = ln_fwd(lib, x, g, b, Bt, E, N * E)
    ok(lib, rc)
    rc, compact = ln_fwd(lib, x[::N].contiguous(), g, b, Bt, E, 0)
    ok(lib, rc)
    for s_, c_ in zip(strided, compact):
        assert same_bits(s_, c_)
    assert same_bits(strided[1][:Bt], yf[:rows:N]) and same_bits(strided[4][:Bt], y8[:rows:N])
    assert guard_intact(strided[0], Bt, E) and guard_intact(strided[1], Bt, E) and bool((strided[4][Bt] == 0x7F).all())


def test_ln_fwd_refuses_the_fp8_copy_at_other_widths(lib):
    E, rows = 132, 4
    x = rnd(rows, E, seed=1); g = rnd(E, seed=2); b = rnd(E, seed=3)
    rc, (yb, yf, mean, rstd, y8) = ln_fwd(lib, x, g, b, rows, E, 0)
    refused(lib, rc, "ln_fwd", "multiple of 128")
    torch.cuda.synchronize()
    assert torch.isnan(yf[:rows]).all()
    rc, outs = ln_fwd(lib, x, g, b, rows, E, 0, fp8=False)           # the width itself is fine
    ok(lib, rc)
    assert torch.isfinite(outs[1][:rows]).all()


# ------------------------------------------------------------------------------------------------ 2c. attention
@pytest.mark.parametrize("H", [2, 4])
@pytest.mark.parametrize("N", [10, 50, 145, 257])
def test_attention_fwd_fp8_copy(lib, N, H):
    """out_fp8 = e4m3 codes of the f32 value that `out` is the bf16 rounding of, k-permuted.  Bound on |dec - out|: half an e4m3
    step is <= 2^-4 relative (3 mantissa bits), half a bf16 step 2^-9, half the smallest e4m3 subnormal 2^-10:
    with o the f32 value, |dec - out| <= (2^-4 + 2^-9) |o| + 2^-10 and |o| <= |out| / (1 - 2^-9), i.e. 0.0646 |out| + 2^-10; the
    required bound is 0.0665 |out| + 2^-10"""
    from pevit_amd import fp8
    Bt = 2
    E, T = H * 64, Bt * N
    q, k, v, _ = (t.cuda() for t in sweep_inputs(N, Bt, H))
    out = guarded(T, E, torch.bfloat16); lse = guarded(1, Bt * H * N, torch.float32)
    o8 = torch.full((T + 1, E), 0x7F, dtype=torch.uint8, device="cuda")
    ok(lib, lib.pevit_op_attn_fwd_ex(S(), P(q), P(k), P(v), P(out), E, P(lse), Bt, H, N, P(o8)))
    plain = guarded(T, E, torch.bfloat16); lse2 = guarded(1, Bt * H * N, torch.float32)
    ok(lib, lib.pevit_op_attn_fwd(S(), P(q), P(k), P(v), P(plain), E, P(lse2), Bt, H, N))
    assert same_bits(out, plain) and same_bits(lse, lse2)           # the copy changes nothing else
    assert guard_intact(out, T, E) and bool((o8[T] == 0x7F).all())
    o = out[:T].float().cpu()
    dec = o8[:T].cpu()[:, fp8.kperm(E)].view(torch.float8_e4m3fn).float()
    assert torch.isfinite(dec).all()
    excess = ((dec - o).abs() - (0.0665 * o.abs() + 2.0 ** -10)).max()
    print(f"\nN={N} H={H}: largest |dec - out| - bound = {float(excess):.3e}; max |dec - out| / |out| = "
          f"{float(((dec - o).abs() / o.abs().clamp_min(2.0 ** -6)).max()):.3e}")
    assert float(excess) <= 0.0


@pytest.mark.parametrize("N", [1, 10, 50, 64])
def test_attention_bwd_class_token_only_dout(lib, N):
    """dout_cls_only: bit-identical to the plain call on a dO that is zero off token 0; the flagged call's other rows hold NaN"""
    Bt, H = SWEEP_BT, SWEEP_H
    E, T, ld = H * 64, Bt * N, 3 * H * 64 + 64
    q, k, v, do = (t.cuda() for t in sweep_inputs(N, Bt, H))
    out = guarded(T, E, torch.bfloat16); lse = guarded(1, Bt * H * N, torch.float32)
    ok(lib, lib.pevit_op_attn_fwd(S(), P(q), P(k), P(v), P(out), E, P(lse), Bt, H, N))
    tok0 = (torch.arange(T, device="cuda") % N == 0)[:, None]
    res = []
    for flag, fill in ((0, 0.0), (1, NAN)):
        d = torch.where(tok0, do, torch.full_like(do, fill))
        dqkv = guarded(T, 3 * E, torch.bfloat16, ld)
        ok(lib, lib.pevit_op_attn_bwd_ex(S(), P(q), P(k), P(v), P(out), E, P(d), E, P(lse), P(dqkv), ld, Bt, H, N, flag))
        assert guard_intact(dqkv, T, 3 * E) and torch.isfinite(dqkv[:T, :3 * E].float()).all()
        res.append(dqkv)
    assert same_bits(res[0], res[1])
    # and the plain call is the attention backward (the gate of test_attention_fwd_bwd)
    _, _, dq, dk, dv = attn_ref64(q, k, v, heads_of(torch.where(tok0, do, torch.zeros_like(do)), Bt, H, N))
    for i, g in enumerate((dq, dk, dv)):
        assert rel_err(res[1][:T, i * E:(i + 1) * E].float(), rows_of(g, Bt, H, N)) < GRAD_GATE


def test_attention_bwd_class_token_only_dout_needs_the_small_kernel(lib):
    Bt, H, N = 1, 2, 65
    E = H * 64
    buf = torch.zeros((Bt * N, 3 * E + 64), dtype=torch.bfloat16, device="cuda")
    qkv = torch.zeros((Bt * H, N, 64), dtype=torch.bfloat16, device="cuda")
    lse = torch.zeros(Bt * H * N, device="cuda")
    refused(lib, lib.pevit_op_attn_bwd_ex(S(), P(qkv), P(qkv), P(qkv), P(buf), E, P(buf), E, P(lse), P(buf), 3 * E + 64, Bt, H, N, 1),
            "attn_bwd", "dout_cls_only", "N = 65")
