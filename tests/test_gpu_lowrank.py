"""The attention-site low-rank adapter kernels (csrc/lowrank.hip and their f32 twins in csrc/verify.hip), one launch at a time through
the test-only pevit_op_lowrank_ex / pevit_op_prep_lowrank / pevit_op_chain_lowrank / pevit_op_rule_sum (csrc/verify.hip: they fill the
launchers' parameter structs by name and add no kernel).  pevit_op_lowrank_plan reports what a launch does on the device found -- the
64-column slabs per gradient workgroup (es), the block ranges, the chunks -- from the code the launchers themselves run.

Inputs, float64 references, the assertions (`check_u`, `check_grad`, `check_reduce`, `check_chain`, `check_rule_sum`, `check_prep`)
and the gates come from tests/test_lowrank_host.py, which proves on the CPU that they bite (ten wrong kernels) and measures the floors:
gate = 2 x max(floor, 2^-24), floor = the same arithmetic with the kernels' rounding points against float64, capped by the existing
gates (2e-4 for u32 and the partials, 2e-5 for pure-f32 outputs, 1e-2 for bf16 panels).

Shapes (B, N, H), E = 64 H: (1,1,1) T = 1; (3,5,1) less than one MFMA row group; (6,10,2); (1,257,2) a one-row second chunk;
(2,128,5) T = 256 exactly, five slabs; (1,50,12), (2,197,12), (1,257,16) the smallest towers on the three compile-time instances of
lowrank_combo; and two shapes found through the plan query: (B,50,12) with the smallest B at which lowrank_grad's es leaves 1, and
(B,257,16) with the smallest B at which it takes a third value (`big_shapes`; on a 256-CU MI355X: B = 72 -> T = 3600, es = 2 and
B = 21 -> T = 5397, es = 4).  test_slab_groupings_exercised names the es values of every launch of the file.

Every output is pre-filled with NaN; buffers carry pad columns and guard rows holding a sentinel that must survive; row T of the
q | k | v columns of dqkv and of xn, t and the u32 operand holds NaN: the kernels clamp to row T - 1 and must never use it.

    lowrank_u      u32 against float64; the bf16 copy in dqkv[:, 3E:3E+64] == bf16(u32) bit for bit; nothing else written
    lowrank_grad   every chunk's four planes and both bias rows against the per-chunk float64 reference; xcd_order 0 == 1 in bits
    lowrank_combo  forms (this_layer, prev) = (1,0), (1,1), (0,1) with previous-layer operands of their own: float64, and the bits of
                   lowrank_grad on the same operands for all four planes and d bias; what a form does not own stays NaN
    f32 twins      lowrank_u_f32, lowrank_grad_f32 on the small shapes
    preps          3 layers, strides larger than compact, bf16 and f32 storage: the WHOLE buffers (pad columns, stride padding, guard)
                   have the bits of the float32 evaluation in the kernels' operation order; float64 gate; LoRA pad columns +0
    reduce, chain  chunks 1 .. 25, 3 layers with padded strides: G has the bits of the documented tree; gradients within the float64
                   chain; NaN in the LoRA pad columns and in the stride padding must not leak
    rule_sum       five ranges with NaN outside the range; (12,24) then (0,12) has the bits of (0,24)

Kernel figures on the MI355X (256 CUs; max-rel against float64, `pytest -s` prints them next to the floors), floor in brackets:

    shape (B,N,H)   T     lowrank_u u32        lowrank_grad partial / d bias (per chunk and plane)       combo u     deferred dP
    (1,1,1)         1     6.9e-8 (6.9e-8)      0 (0) / 0 (0)                                             6.9e-8      0
    (3,5,1)         15    1.0e-7 (9.2e-8)      6.3e-8 (4.8e-8) / 0 (0)                                   1.0e-7      5.3e-8
    (6,10,2)        60    9.1e-8 (1.3e-7)      1.0e-7 (1.0e-7) / 0 (0)                                   9.1e-8      1.3e-7
    (1,257,2)       257   7.2e-8 (1.5e-7)      2.1e-7 (3.5e-7) / 4.7e-8 (4.7e-8)                         7.2e-8      2.4e-7
    (2,128,5)       256   1.3e-7 (2.0e-7)      2.9e-7 (2.6e-7) / 4.9e-8 (3.5e-8)                         7.5e-8      2.5e-7
    (1,50,12)       50    8.1e-8 (3.0e-7)      1.1e-7 (9.8e-8) / 8.0e-9 (8.0e-9)                         1.2e-7      9.9e-8
    (2,197,12)      394   1.0e-7 (4.4e-7)      2.0e-7 (2.8e-7) / 3.9e-8 (4.3e-8)                         9.2e-8      2.6e-7
    (1,257,16)      257   9.1e-8 (4.1e-7)      2.0e-7 (3.0e-7) / 3.7e-8 (3.7e-8)                         1.4e-7      1.6e-7
    (72,50,12)      3600  1.2e-7 (4.6e-7)      2.6e-7 (3.5e-7) / 4.8e-8 (4.8e-8)   es = 2                1.2e-7      2.5e-7
    (21,257,16)     5397  1.1e-7 (5.6e-7)      2.6e-7 (4.4e-7) / 4.2e-8 (5.0e-8)   es = 4                1.9e-7      3.4e-7

    es exercised: 1 (36 of the 40 launch plans), 2 ((72,50,12): lowrank_grad and combo (1,1)), 4 ((21,257,16): the same two); the
    combo forms (1,0) and (0,1) of the two large shapes run es = 1 and still have the bits of lowrank_grad at es = 2 / 4.
    f32 twins: u 6.9e-8 .. 2.0e-7 (== floor), partial 4.5e-8 .. 6.3e-7 (floor 4.5e-8 .. 6.3e-7).
    preps: every buffer bit-identical to the float32 evaluation; bf16 panels 2.0e-3 .. 3.7e-3 of float64 (== floor), f32 <= 9.4e-8.
    reduce: G bit-identical to the tree, 0 .. 1.2e-7 of float64; d bias bit-identical, <= 1.9e-7.  chain: KAdaptation q_left /
    q_right <= 3.4e-7 (floor 1.7e-7 .. 3.1e-7 per case), rule factors <= 2.7e-7; LoRA <= 5.7e-8 (floor 6.3e-8 .. 1.1e-7).
    rule_sum: 3.5e-8 .. 1.5e-7, identical to the float32 emulation's distance.
No case failed and no kernel was changed.
"""
import ctypes as C
import functools

import pytest
import torch

from conftest import max_rel
from test_gpu_kernel_forms import NAN, SENT, S, ok, refused, same_bits
from test_lowrank_host import (ASCALE, BF, CHAIN_LORA_R, F32_GATE, F32_SHAPES, GRID, LORA_R, PANELS, PREP_E, REDUCE_CHUNKS, RULE_RANGES,
                               case, chain_case, chain_gates, check_chain, check_grad, check_prep, check_reduce, check_rule_sum,
                               check_u, chunks_of, floors, floors_cpu, gates, gate_of, grad64, layer_partial, on, prep_case,
                               prep_gates, prep_panels, rule_case, rule_sum32, rule_sum64)

pytestmark = pytest.mark.gpu

PAD = 8                                      # pad columns behind every row (keeps the 16-byte alignment of the rows)
METHOD = dict(kadaptation=0, lora=1)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pevit_amd import _lib
    return _lib.load()


def plan(lib, B, N, E, this_layer=0, prev=0):
    out = (C.c_int32 * 5)()
    assert lib.pevit_op_lowrank_plan(B, N, E, this_layer, prev, out) == 0, lib.pevit_last_error().decode()
    return dict(zip(("es", "nu", "n12", "n0", "chunks"), out))


@functools.lru_cache(maxsize=None)
def _big_shapes(lib_id):
    from pevit_amd import _lib
    lib = _lib.load()
    first = next(B for B in range(1, 400) if plan(lib, B, 50, 768)["es"] != 1)
    seen = {1, plan(lib, first, 50, 768)["es"]}
    second = next(B for B in range(1, 100) if plan(lib, B, 257, 1024)["es"] not in seen)
    return [(first, 50, 12), (second, 257, 16)]


def big_shapes(lib):
    return _big_shapes(0)


def guarded(rows, width, dtype, pitch=None, fill=NAN, extra=1):
    """[rows + extra][pitch]: the payload [rows][width] holds `fill`, the pad columns and the `extra` rows behind it the sentinel"""
    t = torch.full((rows + extra, pitch or width), SENT, dtype=dtype, device="cuda")
    t[:rows, :width] = fill
    return t


@functools.lru_cache(maxsize=None)
def gcase(B, N, H):
    """the case on the GPU with the operand buffers of the launches: never written by a test (outputs are fresh buffers)"""
    c = on(case(B, N, H), "cuda")
    T, E = c["T"], c["E"]
    c["ld"], c["ldx"] = 3 * E + 64 + PAD, E + PAD
    dqkv = guarded(T, 3 * E, BF, pitch=c["ld"], extra=2)              # u columns, pad columns, rows T and T + 1: sentinel
    dqkv[:T, :E], dqkv[:T, E:2 * E], dqkv[:T, 2 * E:3 * E] = c["dq_rows"], c["dk_rows"], c["dv_rows"]
    dqkv[T, :3 * E] = NAN                                             # clamped, never used
    dqkv[:T, 3 * E:3 * E + 64] = NAN                                  # the bf16 copy of u: an output
    c["dqkv"] = dqkv
    for k, w in (("xn", E), ("t", 64), ("u32", 64)):
        buf = guarded(T, w, c[k].dtype, pitch=w + PAD if k == "xn" else w, extra=2)
        buf[:T, :w] = c[k]
        buf[T, :w] = NAN
        c[k + "_buf"] = buf
    # the operands of "the layer processed before": tensors of their own
    c["xn_prev"], c["u32_prev"] = c["dk_rows"], (0.75 * c["t"]).contiguous()
    for k, w in (("xn_prev", E), ("u32_prev", 64)):
        buf = guarded(T, w, c[k].dtype, pitch=w + PAD if k == "xn_prev" else w, extra=2)
        buf[:T, :w] = c[k]
        buf[T, :w] = NAN
        c[k + "_buf"] = buf
    return c


@functools.lru_cache(maxsize=None)
def gfloors(B, N, H):
    return floors_cpu(B, N, H) if (B, N, H) in GRID else floors(gcase(B, N, H))


def outputs(c, f32=False):
    T, E = c["T"], c["E"]
    ch = chunks_of(T)
    return dict(u32=guarded(T, 64, torch.float32, extra=2), partial=guarded(ch, 4 * E * 32, torch.float32),
                dbias=guarded(ch, 2 * E, torch.float32), partial_prev=guarded(ch, 4 * E * 32, torch.float32))


def launch(lib, form, c, out, dqkv=None, xn=None, u32_in=None, **kw):
    """one pevit_op_lowrank_ex launch; returns the dqkv buffer it used (a fresh copy: the u columns are an output)"""
    from pevit_amd._lib import LOWRANK_FORMS, PevitLowrankArgs
    E = c["E"]
    a = PevitLowrankArgs()
    dqkv = c["dqkv"].clone() if dqkv is None else dqkv
    a.form = LOWRANK_FORMS[form]
    a.dqkv, a.ld = dqkv.data_ptr(), dqkv.stride(0)
    a.u_bf16_cols = dqkv.data_ptr() + 3 * E * dqkv.element_size()
    a.qT, a.q32 = c["qT"].data_ptr(), c["q32"].data_ptr()
    xn = c["xn_buf"] if xn is None else xn
    a.xn, a.ldx = xn.data_ptr(), xn.stride(0)
    a.t = c["t_buf"].data_ptr()
    a.u32 = (out["u32"] if u32_in is None else u32_in).data_ptr()
    a.partial, a.dbias_partial = out["partial"].data_ptr(), out["dbias"].data_ptr()
    a.chunks, a.B, a.H, a.N, a.E = chunks_of(c["T"]), c["B"], c["H"], c["N"], E
    a.xcd_order = 1
    for k, v in kw.items():
        setattr(a, k, v.data_ptr() if torch.is_tensor(v) else v)
    ok(lib, lib.pevit_op_lowrank_ex(S(), C.byref(a)))
    return dqkv


def say(tag, fig, fl=None, extra=""):
    print(f"\n{tag}: " + "  ".join(f"{k} {v:.2e}" + (f" (floor {fl[k]:.2e})" if fl and k in fl else "") for k, v in fig.items()) + extra, end="")


def all_shapes(lib):
    return GRID + big_shapes(lib)


def shape_ids():
    return [f"{B}-{N}-{H}" for B, N, H in GRID] + ["big768", "big1024"]


def resolve(lib, i):
    return all_shapes(lib)[i]


def only_u_written(c, dqkv, out):
    """everything but rows < T of the u columns and of u32 is as it was"""
    T, E = c["T"], c["E"]
    before = c["dqkv"].clone()
    before[:T, 3 * E:3 * E + 64] = dqkv[:T, 3 * E:3 * E + 64]
    assert same_bits(dqkv, before), "lowrank_u wrote outside rows < T of the 64 u columns"
    assert bool((out["u32"][T:] == SENT).all()), "a row >= T of u32 was written"


# ------------------------------------------------------------------------------------------------ u
@pytest.mark.parametrize("i", range(len(GRID) + 2), ids=shape_ids())
def test_lowrank_u(lib, i):
    B, N, H = resolve(lib, i)
    c, fl = gcase(B, N, H), gfloors(B, N, H)
    T, E = c["T"], c["E"]
    out = outputs(c)
    dqkv = launch(lib, "u", c, out)
    fig = dict(u=check_u(c, out["u32"][:T], dqkv[:T, 3 * E:3 * E + 64], gates(fl)["u"]))
    only_u_written(c, dqkv, out)
    assert bool(torch.isnan(out["partial"][:-1]).all()) and bool(torch.isnan(out["dbias"][:-1]).all())
    say(f"lowrank_u B={B} N={N} H={H} T={T}", fig, fl)


# ------------------------------------------------------------------------------------------------ gradients
def grad_launch(lib, c, form="grad", xcd_order=1, xn=None, u32_in=None, dqkv=None):
    out = outputs(c)
    launch(lib, form, c, out, xn=xn, u32_in=c["u32_buf"] if u32_in is None else u32_in, dqkv=dqkv, xcd_order=xcd_order)
    assert bool((out["partial"][-1] == SENT).all()) and bool((out["dbias"][-1] == SENT).all()), "the guard chunk was written"
    assert bool(torch.isnan(out["u32"][:c["T"]]).all()), "lowrank_grad wrote u32"
    return out


def planes(c, buf):
    return buf[:-1].view(chunks_of(c["T"]), 4, c["E"], 32)


def rows2(c, buf):
    return buf[:-1].view(chunks_of(c["T"]), 2, c["E"])


@pytest.mark.parametrize("i", range(len(GRID) + 2), ids=shape_ids())
def test_lowrank_grad(lib, i):
    B, N, H = resolve(lib, i)
    c, fl = gcase(B, N, H), gfloors(B, N, H)
    pl = plan(lib, B, N, c["E"])
    assert pl["chunks"] == chunks_of(c["T"]) == lib.pevit_op_lowrank_chunks(c["T"]) and pl["nu"] == 0
    assert pl["n12"] == 2 * pl["n0"] == 2 * pl["chunks"] * (c["E"] // 64 // pl["es"])
    o1, o0 = grad_launch(lib, c, xcd_order=1), grad_launch(lib, c, xcd_order=0)
    fig = check_grad(c, planes(c, o1["partial"]), rows2(c, o1["dbias"]), gates(fl))
    assert same_bits(o1["partial"], o0["partial"]) and same_bits(o1["dbias"], o0["dbias"]), "xcd_order changes bits"
    say(f"lowrank_grad B={B} N={N} H={H} T={c['T']} es={pl['es']}", fig, fl)


@pytest.mark.parametrize("this_layer,prev", [(1, 0), (1, 1), (0, 1)])
@pytest.mark.parametrize("i", range(len(GRID) + 2), ids=shape_ids())
def test_lowrank_combo(lib, i, this_layer, prev):
    B, N, H = resolve(lib, i)
    c, fl = gcase(B, N, H), gfloors(B, N, H)
    T, E = c["T"], c["E"]
    g = gates(fl)
    pl = plan(lib, B, N, E, this_layer, prev)
    out = outputs(c)
    dqkv = launch(lib, "combo", c, out, this_layer=this_layer, prev=prev, xn_prev=c["xn_prev_buf"], u32_prev=c["u32_prev_buf"],
                  partial_prev=out["partial_prev"], xn=c["xn_prev_buf"])
    for k in ("partial", "dbias", "partial_prev"):
        assert bool((out[k][-1] == SENT).all()), f"the guard chunk of {k} was written"
    # lowrank_grad on the operands each range reads: dQ / d bias of this layer, dP of the previous one
    base = grad_launch(lib, c, xn=c["xn_prev_buf"], u32_in=c["u32_prev_buf"])
    fig = {}
    cur, prv, bp = planes(c, out["partial"]), planes(c, out["partial_prev"]), planes(c, base["partial"])
    assert bool(torch.isnan(cur[:, :2]).all()) and bool(torch.isnan(prv[:, 2:]).all()), "a plane that no range owns was written"
    if this_layer:
        fig["u"] = check_u(c, out["u32"][:T], dqkv[:T, 3 * E:3 * E + 64], g["u"])
        only_u_written(c, dqkv, out)
        assert same_bits(cur[:, 2:], bp[:, 2:]) and same_bits(out["dbias"], base["dbias"]), "dQ / d bias: not the bits of lowrank_grad"
        ref = grad64(c)
        full = torch.cat([ref[0][:, :2].float(), cur[:, 2:]], 1)          # (the dP planes of THIS layer are not this launch's)
        fig.update({k: v for k, v in check_grad(c, full, rows2(c, out["dbias"]), g).items()})
    else:
        assert same_bits(dqkv, c["dqkv"]) and bool(torch.isnan(out["u32"][:T]).all()), "form (0,1) wrote u"
        assert bool(torch.isnan(cur).all()) and bool(torch.isnan(out["dbias"][:-1]).all()), "form (0,1) wrote this layer's partials"
    if prev:
        assert same_bits(prv[:, :2], bp[:, :2]), "deferred dP: not the bits of lowrank_grad"
        cp = dict(c, xn=c["xn_prev"], u32=c["u32_prev"])
        fig["dP_prev"] = check_grad(cp, prv, None, g, dp_only=True)["partial"]
    else:
        assert bool(torch.isnan(prv).all()), "partial_prev written without deferred work"
    say(f"lowrank_combo({this_layer},{prev}) B={B} N={N} H={H} T={T} es={pl['es']} nu={pl['nu']} n12={pl['n12']} n0={pl['n0']}", fig, fl)


def test_slab_groupings_exercised(lib):
    """the launches of this file run the slab loop of lowrank_grad_body with one slab per workgroup and with at least two larger
    groupings (register prefetch of the next slab, LDS reuse)"""
    seen = {}
    for B, N, H in all_shapes(lib):
        for form in ((0, 0), (1, 0), (1, 1), (0, 1)):
            seen.setdefault(plan(lib, B, N, 64 * H, *form)["es"], []).append((B, N, H) + form)
    print("\nes values exercised: " + "; ".join(f"es={k}: {len(v)} launches, e.g. (B,N,H,this_layer,prev)={v[0]}" for k, v in sorted(seen.items())), end="")
    assert 1 in seen and len([k for k in seen if k > 1]) >= 2, sorted(seen)


# ------------------------------------------------------------------------------------------------ f32 twins
@pytest.mark.parametrize("B,N,H", F32_SHAPES)
def test_f32_twins(lib, B, N, H):
    c = gcase(B, N, H)
    T, E = c["T"], c["E"]
    fl = floors(case(B, N, H), f32_operands=True)
    g = gates(fl, F32_GATE)
    ld = 3 * E + 64 + 4
    dqkv = guarded(T, 3 * E, torch.float32, pitch=ld, extra=2)
    dqkv[:T, :3 * E] = c["dqkv"][:T, :3 * E].float()
    before = dqkv.clone()
    xn = guarded(T, E, torch.float32, pitch=E + 4)
    xn[:T, :E] = c["xn"].float()
    out = outputs(c)
    launch(lib, "u_f32", c, out, dqkv=dqkv)
    fig = dict(u=check_u(c, out["u32"][:T], None, g["u"]))
    assert same_bits(dqkv[:T, 3 * E:3 * E + 64], out["u32"][:T]), "the second copy of u differs"
    before[:T, 3 * E:3 * E + 64] = dqkv[:T, 3 * E:3 * E + 64]
    assert same_bits(dqkv, before) and bool((out["u32"][T:] == SENT).all())
    out = outputs(c)
    launch(lib, "grad_f32", c, out, dqkv=before, xn=xn, u32_in=c["u32_buf"])
    assert bool((out["partial"][-1] == SENT).all()) and bool((out["dbias"][-1] == SENT).all())
    fig.update(check_grad(c, planes(c, out["partial"]), rows2(c, out["dbias"]), g, f32_operands=True))
    say(f"f32 twins B={B} N={N} H={H}", fig, fl)


def test_null_structs_are_refused(lib):
    refused(lib, lib.pevit_op_lowrank_ex(S(), None), "lowrank_ex", "null argument struct")
    refused(lib, lib.pevit_op_prep_lowrank(S(), None), "prep_lowrank", "null argument struct")
    refused(lib, lib.pevit_op_chain_lowrank(S(), None), "chain_lowrank", "null argument struct")


# ------------------------------------------------------------------------------------------------ preps
def prep_buffers(c, f32):
    """five byte buffers of L strides + a guard, every byte 0xFF (bf16 and f32 NaN); returns them with the geometry"""
    E, L = c["E"], c["L"]
    es = 4 if f32 else 2
    ldw, ldwT = E + PAD, 64 + PAD
    size = dict(w_aug_rows=64 * ldw * es, wT_aug_cols=E * ldwT * es, q32=E * 64 * 4, qT=64 * E * es, q16=E * 64 * 2)
    arena = max(size.values()) + 256
    return {k: torch.full((L * arena + 256,), 0xFF, dtype=torch.uint8, device="cuda") for k in PANELS}, arena, ldw, ldwT


def panel_view(buf, l, arena, rows, cols, pitch, dtype):
    es = torch.empty((), dtype=dtype).element_size()
    return buf[l * arena:l * arena + rows * pitch * es].view(dtype).view(rows, pitch)[:, :cols]


def prep_launch(lib, c, f32, bufs, arena, ldw, ldwT, E=None, r=None):
    from pevit_amd._lib import PevitPrepLowrankArgs
    a = PevitPrepLowrankArgs()
    a.method, a.layers, a.E, a.r, a.f32, a.ldw, a.ldwT = METHOD[c["method"]], c["L"], E or c["E"], c["r"] if r is None else r, int(f32), ldw, ldwT
    a.ascale, a.arena_bytes, a.param_floats = ASCALE, arena, c["param_floats"]
    rule, lp = c["rule"].cuda().contiguous(), c["layer_params"].cuda().contiguous()
    a.rule1_l, a.rule1_r, a.rule2_l, a.rule2_r = (rule[i].data_ptr() for i in range(4))
    rE = c["r"] * c["E"]
    a.q_left, a.q_right = lp.data_ptr(), lp.data_ptr() + 4 * c["E"]
    a.a1q, a.a2q, a.a1v, a.a2v = (lp.data_ptr() + 4 * i * rE for i in range(4))
    for k in PANELS:
        setattr(a, k, bufs[k].data_ptr())
    rc = lib.pevit_op_prep_lowrank(S(), C.byref(a))
    torch.cuda.synchronize()
    return rc


PREP_CASES = [(E, "kadaptation", 32) for E in PREP_E] + [(E, "lora", r) for E in PREP_E for r in LORA_R]


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("E,method,r", PREP_CASES)
def test_prep(lib, E, method, r, f32):
    c = prep_case(E, method, r)
    bufs, arena, ldw, ldwT = prep_buffers(c, f32)
    expect = {k: b.clone() for k, b in bufs.items()}
    ok(lib, prep_launch(lib, c, f32, bufs, arena, ldw, ldwT))
    st = torch.float32 if f32 else BF
    geom = dict(w_aug_rows=(64, E, ldw, st), wT_aug_cols=(E, 64, ldwT, st), q32=(E, 64, 64, torch.float32), qT=(64, E, E, st), q16=(E, 64, 64, BF))
    gate = prep_gates(c, f32)
    fig = {}
    for l in range(c["L"]):
        emu = prep_panels(c, l, f32=f32)
        for k, e in emu.items():
            panel_view(expect[k], l, arena, *geom[k]).copy_(e.cuda())
        got = {k: panel_view(bufs[k], l, arena, *geom[k]).cpu() for k in emu}
        for k, v in check_prep(c, l, got, f32, gate).items():
            fig[k] = max(fig.get(k, 0.0), v)
    for k in PANELS:                       # pad columns, the padding between the layers, the guard, q16 under f32 storage
        assert torch.equal(bufs[k], expect[k]), f"{k}: a byte outside the panels was written, or a panel is not where its layer stride puts it"
    say(f"prep {method} E={E} r={r} {'f32' if f32 else 'bf16'}", fig)


def test_prep_refusals(lib):
    ck, cl = prep_case(64, "kadaptation"), prep_case(64, "lora", 4)
    bufs, arena, ldw, ldwT = prep_buffers(ck, False)
    before = {k: b.clone() for k, b in bufs.items()}
    refused(lib, prep_launch(lib, ck, False, bufs, arena, ldw, ldwT, E=48), "prep_kadapt", "width 48 not divisible by phm_dim 32")
    refused(lib, prep_launch(lib, cl, False, bufs, arena, ldw, ldwT, r=0), "prep_lora", "rank 0 outside [1,32]")
    refused(lib, prep_launch(lib, cl, False, bufs, arena, ldw, ldwT, r=33), "prep_lora", "rank 33 outside [1,32]")
    for k in PANELS:
        assert torch.equal(bufs[k], before[k]), k


# ------------------------------------------------------------------------------------------------ reduce and chain rules
CHAIN_CASES = [(E, ch, "kadaptation", 32) for E in PREP_E for ch in REDUCE_CHUNKS] + \
              [(E, ch, "lora", r) for E in PREP_E for ch in REDUCE_CHUNKS for r in CHAIN_LORA_R]


@pytest.mark.parametrize("E,chunks,method,r", CHAIN_CASES)
def test_reduce_and_chain(lib, E, chunks, method, r):
    from pevit_amd._lib import PevitChainLowrankArgs
    c = chain_case(E, chunks, method, r)
    L, kad = c["L"], method == "kadaptation"
    gG, gb, gchain = chain_gates(E, chunks, method, r)
    partial, dbias, params, grads = (c[k].cuda() for k in ("partial", "dbias", "params", "grads0"))
    G = guarded(L, 4 * E * 32, torch.float32)
    scratch = guarded(L, 4096, torch.float32)
    a = PevitChainLowrankArgs()
    a.method, a.chunks, a.layers, a.E, a.r, a.ascale = METHOD[method], chunks, L, E, r, ASCALE
    a.partial, a.partial_layer, a.G, a.grads = partial.data_ptr(), c["partial_layer"], G.data_ptr(), grads.data_ptr()
    a.p_layer0, a.p_layer_stride = c["p_layer0"], c["p_layer_stride"]
    if kad:
        a.dbias_partial, a.dbias_layer, a.rule_scratch, a.params = dbias.data_ptr(), c["dbias_layer"], scratch.data_ptr(), params.data_ptr()
    ok(lib, lib.pevit_op_chain_lowrank(S(), C.byref(a)))
    assert bool((G[-1] == SENT).all()) and bool((scratch[-1] == SENT).all()), "a guard row was written"
    if not kad:
        assert bool(torch.isnan(scratch[:-1]).all()), "the LoRA chain wrote rule_scratch"
    fig = {}
    for l in range(L):
        part, db = layer_partial(c, l)
        o = c["p_layer0"] + l * c["p_layer_stride"] + 4 * E
        f = check_reduce(G[l].cpu(), part, grads[o:o + E].cpu() if kad else None, db, c["grads0"][o:o + E] if kad else None, gG, gb, cols=r)
        for k, v in f.items():
            fig[k] = max(fig.get(k, 0.0), v)
    fig.update(check_chain(c, grads, scratch[:-1], torch.nan_to_num(G[:-1].view(L, 4, E, 32)), gchain))
    say(f"chain {method} E={E} chunks={chunks} r={r}", fig)


# ------------------------------------------------------------------------------------------------ rule_sum
def rule_launch(lib, scratch, grads, l_lo, l_hi):
    ok(lib, lib.pevit_op_rule_sum(S(), C.c_void_p(scratch.data_ptr()), C.c_void_p(grads.data_ptr()), l_lo, l_hi))


def rule_buffers(l_lo, l_hi):
    rc = rule_case()
    scratch = rc["scratch"].clone()
    scratch[:l_lo] = NAN
    scratch[l_hi:] = NAN
    grads = torch.full((4096 + 16,), SENT)
    grads[:4096] = rc["start"]
    return rc, scratch.cuda(), grads.cuda()


@pytest.mark.parametrize("l_lo,l_hi", RULE_RANGES)
def test_rule_sum(lib, l_lo, l_hi):
    rc, scratch, grads = rule_buffers(l_lo, l_hi)
    rule_launch(lib, scratch, grads, l_lo, l_hi)
    assert bool((grads[4096:] == SENT).all())
    floor = max_rel(rule_sum32(rc["scratch"], rc["start"], l_lo, l_hi), rule_sum64(rc["scratch"], rc["start"], l_lo, l_hi))
    fig = dict(rule_sum=check_rule_sum(grads[:4096].cpu(), rc["scratch"], rc["start"], l_lo, l_hi, gate_of(floor, F32_GATE)))
    say(f"rule_sum [{l_lo}, {l_hi})", fig, dict(rule_sum=floor))


def test_rule_sum_in_two_ranges_from_the_top_has_the_bits_of_one_call(lib):
    rc, scratch, one = rule_buffers(0, 24)
    rule_launch(lib, scratch, one, 0, 24)
    two = one.clone()
    two[:4096] = rc["start"].cuda()
    rule_launch(lib, scratch, two, 12, 24)
    rule_launch(lib, scratch, two, 0, 12)
    assert same_bits(one, two)
