"""adapter_fwd_kernel / adapter_bwd_kernel (csrc/adapter_fused.hip), one launch at a time through the test-only
pevit_op_adapter_fwd_ex / pevit_op_adapter_bwd_ex (csrc/verify.hip: they fill AdapterFwdArgs / AdapterBwdArgs by name and call the
production launchers; they add no kernel).  The towers of the suite reach these kernels at width 256 and 768 with the bf16 gradient
stream only; here every instance the launchers can select is launched and held to float64:

    forward   <act, NV>            (ReLU | gelu_new) x (NV = E / 256 = 1..4)                       8 instances
    backward  <act, RES16, NV>     ... x (RES16 = dres absent | f32 dres given)                   16 instances

    instance -> cases (test_forward / test_backward, ids [E-act-T] and [E-act-residual-T]):
      fwd <ReLU, 1..4>             E = 256, 512, 768, 1024, act 0, every T of (1, 33, 64, 70); E = 768 and 1024 also T = 8229
      fwd <gelu_new, 1..4>         the same with act 1
      bwd <ReLU, RES16, 1..4>      E = 256 .. 1024, act 0, residual "bf16", every T; also the contraction-range cases (E = 256, 1024)
      bwd <ReLU, f32 dres, 1..4>   E = 256 .. 1024, act 0, residual "f32", every T; also test_residual_operand
      bwd <gelu_new, RES16, 1..4>  E = 256 .. 1024, act 1, residual "bf16", every T
      bwd <gelu_new, f32, 1..4>    E = 256 .. 1024, act 1, residual "f32", every T; also test_residual_operand

T: 1 = a single row; 33 = a one-row second tile; 64 = exact tiles; 70 = a 6-row last tile; 8229 = 32 x 257 + 5, more workgroups
than CUs at one workgroup per CU (E = 768, 1024).

Inputs, float64 references and the assertions themselves (`check_forward`, `check_backward`, `bf16_close`) come from
tests/test_adapter_fused_host.py, which also proves on the CPU that they bite (seven wrong kernels) and that a float32 stand-in for a
correct kernel stays 10x inside their cap.  Every stage is checked against float64 of the operands the SAME launch stored for the
stage before it; the backward's saved activation and LayerNorm statistics come from the float64 forward, not from the forward kernel.
Gates: f32 outputs 2e-5 max-rel (test_layernorm_fwd_bwd), column sums 1e-4 block by block (test_ln_bwd_affine), bf16 outputs
bf16_close, and end to end x_out and act within 2x the emulation's rounding floor of the same case against the pure float64
reference (CPU floors at T = 70: x_out 7e-4 .. 1.2e-3, act 2.8e-3 .. 5.2e-3; at T = 1: x_out 4.4e-4 .. 8.0e-4, act 1.4e-3 .. 4.5e-3).

Kernel figures on the MI355X: none recorded yet -- every test prints its figures next to the floors (`pytest -s`).

Every output buffer is pre-filled with NaN (an unwritten element fails) and is followed by 32 guard rows holding a sentinel (the
pad rows of a ragged 32-row tile must not be stored); the ReLU forward gets a NaN-filled apre that must come back untouched.

The folded contraction range (af_tn_range: the two token-contracted weight-gradient products as extra workgroups of the backward
launch) is run with product 1 alone and with both products, with one workgroup per unit pair (tn_blocks = 0) and with 1 and 3
walking workgroups (several trips, unequal trip counts at 3), at 1, 2 and 3 chunks with a ragged last one: its outputs must have the
bits of pevit_op_tn_gemm64 on the same operands, and dpre / dh / partial the bits of the launch without the range.
"""
import ctypes as C
import functools

import pytest
import torch

from conftest import max_rel
from test_adapter_fused_host import (ACTS, BIG_T, COLSUM_GATE, FLOOR_FACTOR, GRID_E, GRID_T, ROWS, case,
                                     check_backward, check_forward, floors, forward64, on, stored)
from test_gpu_kernel_forms import NAN, SENT, P, S, bits, ok, refused, same_bits

pytestmark = pytest.mark.gpu

GUARD = ROWS                     # guard rows behind every row-indexed output: a whole tile's worth of pad rows
BF = torch.bfloat16
FWD_CASES = [(E, a, T) for E in GRID_E for a in ACTS for T in GRID_T] + [(E, a, BIG_T) for E in (768, 1024) for a in ACTS]
RANGE_E, RANGE_T = (256, 1024), (70, 300, 513)          # 1, 2 and 3 chunks of 256 rows, the last one ragged


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pevit_amd import _lib
    return _lib.load()


def guarded(rows, width, dtype, guard=GUARD):
    """[rows + guard][width]: the payload rows hold NaN, the guard rows the sentinel"""
    t = torch.full((rows + guard, width), SENT, dtype=dtype, device="cuda")
    t[:rows] = NAN
    return t


def intact(t, rows):
    return bool((t[rows:] == SENT).all())


@functools.lru_cache(maxsize=None)
def gcase(E, T):
    return on(case(E, T), "cuda")


@functools.lru_cache(maxsize=None)
def gbwd(E, T, act_kind):
    """saved, mean_a, rstd_a and a z operand, from the float64 forward on the GPU (never from the forward kernel)"""
    f = stored(forward64(gcase(E, T), act_kind))
    return f["act" if act_kind == 0 else "apre"].contiguous(), f["mean_a"].contiguous(), f["rstd_a"].contiguous(), f["z"].contiguous()


@functools.lru_cache(maxsize=None)
def gfloor(E, T, act_kind):
    fl, pure = floors(gcase(E, T), act_kind)
    return fl, {k: pure[k] for k in fl}


def launch_fwd(lib, c, act_kind):
    from pevit_amd._lib import PevitAdapterFwdArgs
    T, E = c["T"], c["E"]
    buf = dict(z=guarded(T, E, BF), mean_a=guarded(T, 1, torch.float32), rstd_a=guarded(T, 1, torch.float32),
               act=guarded(T, 64, BF), apre=guarded(T, 64, BF), x_out=guarded(T, E, torch.float32))
    a = PevitAdapterFwdArgs()
    a.act_kind, a.T, a.E = act_kind, T, E
    for k in ("hraw", "bpr", "x_mid", "gamma", "beta", "wd", "b_down", "wu", "b_up"):
        assert c[k].is_contiguous()
        setattr(a, k, c[k].data_ptr())
    for k, t in buf.items():
        setattr(a, k, t.data_ptr())
    ok(lib, lib.pevit_op_adapter_fwd_ex(S(), C.byref(a)))
    return buf


def fwd_payload(buf, T, act_kind):
    for k, t in buf.items():
        assert intact(t, T), f"{k}: a row >= T was written"
    if act_kind == 0:            # only the gelu_new instance writes the pre-activation
        assert bool(torch.isnan(buf["apre"][:T].float()).all()), "the ReLU forward wrote apre"
    got = {k: t[:T] for k, t in buf.items() if not (k == "apre" and act_kind == 0)}
    got["mean_a"], got["rstd_a"] = got["mean_a"].view(-1), got["rstd_a"].view(-1)
    for k, t in got.items():
        assert bool(torch.isfinite(t.float()).all()), f"{k}: an element was left unwritten"
    return got


def launch_bwd(lib, c, act_kind, ops, dres, tn=None, tn_blocks=0):
    """ops = (saved, mean_a, rstd_a); dres: the f32 residual gradient or None; tn: dict of tn_* operands / outputs"""
    from pevit_amd._lib import PevitAdapterBwdArgs
    T, E = c["T"], c["E"]
    nb = lib.pevit_op_adapter_blocks(T)
    buf = dict(dpre=guarded(T, 64, BF), dh_bf16=guarded(T, E, BF), partial=guarded(nb, 3 * E, torch.float32, guard=1))
    a = PevitAdapterBwdArgs()
    a.act_kind, a.T, a.E, a.tn_blocks = act_kind, T, E, tn_blocks
    for k in ("dyb", "wuT", "wdT", "hraw", "bpr", "gamma"):
        assert c[k].is_contiguous()
        setattr(a, k, c[k].data_ptr())
    a.saved, a.mean_a, a.rstd_a = (t.data_ptr() for t in ops)
    a.dres = None if dres is None else dres.data_ptr()
    for k, t in buf.items():
        setattr(a, k, t.data_ptr())
    for k, t in (tn or {}).items():
        setattr(a, k, t.data_ptr())
    rc = lib.pevit_op_adapter_bwd_ex(S(), C.byref(a))
    return rc, buf, nb


def bwd_payload(buf, T, E, nb):
    assert intact(buf["dpre"], T) and intact(buf["dh_bf16"], T), "a row >= T of dpre / dh was written"
    assert intact(buf["partial"], nb), "a block >= pevit_op_adapter_blocks(T) of partial was written"
    got = dict(dpre=buf["dpre"][:T], dh=buf["dh_bf16"][:T], partial=buf["partial"][:nb].view(nb, 3, E))
    for k, t in got.items():
        assert bool(torch.isfinite(t.float()).all()), f"{k}: an element was left unwritten"
    return got


def say(tag, fig):
    print(f"\n{tag}: " + "  ".join(f"{k} {v:.2e}" for k, v in fig.items()), end="")


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("E,act_kind,T", FWD_CASES)
def test_forward(lib, E, act_kind, T):
    c = gcase(E, T)
    got = fwd_payload(launch_fwd(lib, c, act_kind), T, act_kind)
    fig = check_forward(got, c, act_kind)
    fl, pure = gfloor(E, T, act_kind)
    for k in ("x_out", "act"):                                   # end to end against the pure reference: the emulation's floor x 2
        fig[f"{k}/pure"] = max_rel(got[k], pure[k])
        fig[f"{k} floor"] = fl[k]
    say(f"fwd E={E} act={act_kind} T={T}", fig)
    for k in ("x_out", "act"):
        assert fig[f"{k}/pure"] <= FLOOR_FACTOR * fl[k], (k, fig)


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("residual", ["f32", "bf16"])
@pytest.mark.parametrize("E,act_kind,T", FWD_CASES)
def test_backward(lib, E, act_kind, T, residual):
    c = gcase(E, T)
    saved, mean_a, rstd_a, _ = gbwd(E, T, act_kind)
    dres = c["dres"] if residual == "f32" else None
    rc, buf, nb = launch_bwd(lib, c, act_kind, (saved, mean_a, rstd_a), dres)
    ok(lib, rc)
    assert nb == -(-T // ROWS)
    got = bwd_payload(buf, T, E, nb)
    fig = check_backward(got, c, act_kind, saved, mean_a, rstd_a, c["dres"] if dres is not None else c["dyb"])
    say(f"bwd E={E} act={act_kind} T={T} res={residual}", fig)


@pytest.mark.parametrize("act_kind", ACTS)
@pytest.mark.parametrize("E", GRID_E)
def test_residual_operand(lib, E, act_kind):
    """dres = f32(dyb) + 0.25 breaks the production relation dyb = bf16(dres): with dres given, the residual of dh and the d b_up
    sums (sum 2) carry the offset; without it they come from dyb -- while the products take dyb in both"""
    T = 70
    c = dict(gcase(E, T))
    c["dres"] = c["dyb"].float() + 0.25
    saved, mean_a, rstd_a, _ = gbwd(E, T, act_kind)
    res = {}
    for name, dres in (("f32", c["dres"]), ("bf16", None)):
        rc, buf, nb = launch_bwd(lib, c, act_kind, (saved, mean_a, rstd_a), dres)
        ok(lib, rc)
        res[name] = bwd_payload(buf, T, E, nb)
        check_backward(res[name], c, act_kind, saved, mean_a, rstd_a, c["dres"] if dres is not None else c["dyb"])
    rows = torch.tensor([min(ROWS, T - ROWS * b) for b in range(nb)], dtype=torch.float64, device="cuda").view(nb, 1)
    shift = res["f32"]["partial"][:, 2].double() - res["bf16"]["partial"][:, 2].double()
    assert float((shift - 0.25 * rows).abs().max()) < COLSUM_GATE * float(res["bf16"]["partial"][:, 2].abs().max())
    assert abs(float((res["f32"]["dh"].double() - res["bf16"]["dh"].double()).mean()) - 0.25) < 2.0 ** -9      # bf16 rounding of dh, averaged


# ------------------------------------------------------------------------------------------------ the folded contraction range
def tn_reference(lib, X, Y, T, E, with_csy):
    ch = lib.pevit_op_tn_chunks(T)
    partial = guarded(ch, E * 64, torch.float32, guard=1)
    csy = guarded(ch, 64, torch.float32, guard=1)
    ok(lib, lib.pevit_op_tn_gemm64(S(), P(X), E, P(Y), 64, P(partial), None, P(csy) if with_csy else None, T, E))
    return partial, csy


@pytest.mark.parametrize("T", RANGE_T)
@pytest.mark.parametrize("E", RANGE_E)
def test_contraction_range_has_the_bits_of_tn_gemm64(lib, E, T):
    act_kind = 0
    c = gcase(E, T)
    saved, mean_a, rstd_a, z = gbwd(E, T, act_kind)
    ops = (saved, mean_a, rstd_a)
    g = torch.Generator(device="cpu").manual_seed(7 * E + T)
    y2 = (torch.randn(T, 64, generator=g) * 0.5).to(BF).cuda()          # a d pre of another layer: not the buffer this launch writes
    ch = lib.pevit_op_tn_chunks(T)
    assert ch == -(-T // 256)
    ref1, _ = tn_reference(lib, c["dyb"], saved, T, E, False)
    ref2, refcs = tn_reference(lib, z, y2, T, E, True)
    rc, base, nb = launch_bwd(lib, c, act_kind, ops, None)
    ok(lib, rc)
    bwd_payload(base, T, E, nb)
    for both in (False, True):
        for tn_blocks in (0, 1, 3):
            tn = dict(tn_x1=c["dyb"], tn_y1=saved, tn_partial1=guarded(ch, E * 64, torch.float32, guard=1))
            if both:
                tn.update(tn_x2=z, tn_y2=y2, tn_partial2=guarded(ch, E * 64, torch.float32, guard=1),
                          tn_csy2=guarded(ch, 64, torch.float32, guard=1))
            rc, buf, nb = launch_bwd(lib, c, act_kind, ops, None, tn, tn_blocks)
            ok(lib, rc)
            what = f"products {'1+2' if both else '1'}, tn_blocks={tn_blocks}"
            assert same_bits(tn["tn_partial1"], ref1), what
            if both:
                assert same_bits(tn["tn_partial2"], ref2) and same_bits(tn["tn_csy2"], refcs), what
            for k in base:
                assert same_bits(buf[k], base[k]), (what, k)
    # the deferred product must not read the d pre buffer this launch writes
    dpre = guarded(T, 64, BF)
    from pevit_amd._lib import PevitAdapterBwdArgs
    a = PevitAdapterBwdArgs()
    a.T, a.E = T, E
    a.tn_x2, a.tn_y2, a.dpre = z.data_ptr(), dpre.data_ptr(), dpre.data_ptr()
    refused(lib, lib.pevit_op_adapter_bwd_ex(S(), C.byref(a)), "adapter_bwd", "deferred contraction reads the d pre buffer")
    torch.cuda.synchronize()
    assert bool(torch.isnan(dpre[:T].float()).all()) and intact(dpre, T)


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("act_kind", ACTS)
@pytest.mark.parametrize("E", GRID_E)
def test_two_launches_give_the_same_bits(lib, E, act_kind):
    """every reduction is fixed-order: LDS partial products, wave sums, the column sums of the block"""
    T = 70
    c = gcase(E, T)
    saved, mean_a, rstd_a, _ = gbwd(E, T, act_kind)
    f1, f2 = launch_fwd(lib, c, act_kind), launch_fwd(lib, c, act_kind)
    for k in f1:
        assert same_bits(f1[k], f2[k]), k
    for dres in (c["dres"], None):
        (rc1, b1, _), (rc2, b2, _) = (launch_bwd(lib, c, act_kind, (saved, mean_a, rstd_a), dres) for _ in range(2))
        ok(lib, rc1 or rc2)
        for k in b1:
            assert same_bits(b1[k], b2[k]), (k, dres is None)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("E,T", [(128, 8), (320, 8), (1280, 8), (256, 0)])
def test_unsupported_shapes_are_refused_before_any_launch(lib, E, T):
    from pevit_amd._lib import PevitAdapterBwdArgs, PevitAdapterFwdArgs
    assert lib.pevit_op_adapter_fused_ok(E) == (1 if E == 256 else 0)
    rows = 8
    ins = torch.zeros((rows, 1280), device="cuda")
    outs = {k: guarded(rows, 1280, torch.float32) for k in ("z", "mean_a", "rstd_a", "act", "apre", "x_out", "dpre", "dh_bf16", "partial")}
    before = {k: t.clone() for k, t in outs.items()}
    f = PevitAdapterFwdArgs()
    f.T, f.E = T, E
    for k in ("hraw", "bpr", "x_mid", "gamma", "beta", "wd", "b_down", "wu", "b_up"):
        setattr(f, k, ins.data_ptr())
    for k in ("z", "mean_a", "rstd_a", "act", "apre", "x_out"):
        setattr(f, k, outs[k].data_ptr())
    b = PevitAdapterBwdArgs()
    b.T, b.E = T, E
    for k in ("dyb", "dres", "wuT", "saved", "wdT", "hraw", "bpr", "mean_a", "rstd_a", "gamma"):
        setattr(b, k, ins.data_ptr())
    for k in ("dpre", "dh_bf16", "partial"):
        setattr(b, k, outs[k].data_ptr())
    for act_kind in ACTS:
        f.act_kind = b.act_kind = act_kind
        refused(lib, lib.pevit_op_adapter_fwd_ex(S(), C.byref(f)), "adapter_fwd", "unsupported shape", f"T={T}", f"E={E}")
        refused(lib, lib.pevit_op_adapter_bwd_ex(S(), C.byref(b)), "adapter_bwd", "unsupported shape", f"T={T}", f"E={E}")
    torch.cuda.synchronize()
    for k in outs:
        assert torch.equal(bits(outs[k]), bits(before[k])), k


def test_fused_ok_names_the_four_widths(lib):
    assert [E for E in range(64, 2049, 64) if lib.pevit_op_adapter_fused_ok(E)] == list(GRID_E)
    assert [lib.pevit_op_adapter_blocks(T) for T in (1, 32, 33, 64, 70, BIG_T)] == [1, 1, 2, 2, 3, 258]
