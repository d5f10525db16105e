"""Every GEMM epilogue on every kernel family and operand form that the family units of gemm.hip (gemm_tile.hip, gemm_stag8.hip,
gemm_split.hip, gemm_streamk.hip, gemm_skinny.hip) instantiate, bit for bit.

Everything runs through the test-only pevit_op_gemm_ex (csrc/ops.hip: it fills GemmParams by name, takes a tune of its own --
the process-wide default tune is never touched -- and the caller's stream-K workspace).  The case table, the operands and the
float64 references come from tests/test_gemm_forms_host.py, which also asks the planner itself (csrc/gemm_plan.hip, no GPU needed) for
the family of every case, and proves on the CPU that the operands make every sum exact in
f32 and that the comparison sees the faults it is meant to see.

Gates.  Linear outputs (f32, and bf16 as round-to-nearest-even of an exact value -- the pre-activation h of the GELU epilogues and
relu included): BIT EQUALITY with the float64 reference, on every family, also on those that split the summation (k-split, phased
k-split, stream-K, few rows, two K slices per tile).  Nonlinear outputs: g of QuickGELU / gelu_new against float64 on the kernel's
own stored bf16 h, the three derivative epilogues against float64 on aux, at 1e-2 of the largest magnitude (tests/test_gpu_ops.py);
GELU_ONLY's g is bit-identical to BIAS_GELU's.  Largest deviation over all cases of an epilogue: NOT MEASURED on an MI355X yet (this
file has not run on a device; `pytest -s` prints the figures with the last test, to be recorded here).  For orientation only, float64
rounded to bf16 -- no kernel involved -- gives on these operands: BIAS_GELU 3.3e-4, BIAS_GELUNEW 3.9e-4, DGELU 2.9e-3, DRELU 3.7e-3,
DGELUNEW 3.0e-3.  The gate is the project's, not derived from either.

Buffers.  Every output is a guarded buffer: payload pre-filled with NaN, pad columns and a guard row holding a sentinel that must
survive; residual, positional table and aux carry NaN in their pad columns and guard row.  All pitches of a launch are pairwise
different and none equals a width (the in-place cases share the residual's pitch by construction).  A is a row-strided view whose
row M and pad columns hold NaN; B has b_rows > N with NaN rows [N, b_rows).  For PATCH_EMBED row 0 of every image is part of the
guard.  After every launch the family the planner took is asserted (pevit_debug_last_gemm_path): a planner that does not take the
named family fails the case, nothing skips.  After every launch with the workspace, all hand-off flags / tickets and the stream-K
error word must be zero.

The table against the code: every combination the host table marks as existing is launched and must succeed; every absent one is
asked for -- the planner refuses (rc -1, its own message, outputs untouched) or takes another family (then the result is checked all
the same).  The planner's argument refusals are asserted the same way; nothing here is launched in order to fail.

Shapes assume 256 CUs, like the path assertions of test_gpu_ops.py.
"""
import ctypes as C
import functools
import types

import pytest
import torch

from conftest import max_rel
from pevit_amd._lib import PevitGemmExArgs
from test_gemm_forms_host import (ABSENT, BIAS_GELU, BIAS_GELUNEW, BIAS_RESID, CASES, DGELU, DGELUNEW, DRELU, EPI_NAMES, F32, GELU_ONLY,
                                  KEEP, LINEAR_BF16, LINEAR_F32, NONLINEAR_GATE, OPS_BF16, OPS_FP8A, OPS_FP8B, OPS_TAIL, PATCH, QKV,
                                  TAIL_ROWS, VARIANTS, Case, absent_outcome, activation, case_id, geometry, operands, path_of, pitches,
                                  reference)

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -7.0                      # sentinel of pad columns and guard rows (exact in bf16)
FP8_NAN = 0x7F                   # e4m3fn NaN
MEASURED = {}                    # epilogue -> largest nonlinear deviation of this run (printed by the last test)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pevit_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def ws(lib):
    """the stream-K workspace, sized as op_sk_workspace (ops.hip) sizes it: one flag word per slot + the error word, one 128x128 f32
    slab per slot.  The slabs start as NaN: a partial tile read before it was written shows."""
    slots = lib.pevit_op_gemm_sk_slots()
    assert 8 <= slots <= 1024 and slots % 8 == 0
    return types.SimpleNamespace(slots=slots, flag=torch.zeros(slots + 1, dtype=torch.int32, device="cuda"),
                                 slab=torch.full((slots * 128 * 128,), NAN, device="cuda"))


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def guarded(rows, width, dtype, pitch):
    """[rows + 1][pitch]: the payload [rows][width] holds NaN, the pad columns and the guard row the sentinel"""
    t = torch.full((rows + 1, pitch), SENT, dtype=dtype, device="cuda")
    t[:rows, :width] = NAN
    return t


def guard_intact(t, rows, width):
    return bool((t[rows:] == SENT).all()) and bool((t[:rows, width:] == SENT).all())


def padded_input(values, pitch, dtype):
    """an operand the epilogue reads: [rows + 1][pitch], NaN outside the payload"""
    rows, width = values.shape
    t = torch.full((rows + 1, pitch), NAN, dtype=dtype, device="cuda")
    t[:rows, :width] = values.to(dtype)
    return t


# ------------------------------------------------------------------------------------------------ operands on the device (shared)
@functools.lru_cache(maxsize=3)
def problem(M, N, K, ops):
    """operands() on the GPU plus the exact float64 product; computed once per problem, never modified"""
    d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in operands(M, N, K, ops).items()}
    d["acc"] = d["A"].double() @ d["W"].double().T
    return d


@functools.lru_cache(maxsize=4)
def a_buffer(M, N, K, ops, lda):
    d = problem(M, N, K, ops)
    if ops == OPS_FP8A:
        buf = torch.full((M + 1, lda), FP8_NAN, dtype=torch.uint8, device="cuda")
        buf[:M, :K] = d["acodes"]
    else:
        buf = torch.full((M + 1, lda), NAN, dtype=torch.bfloat16, device="cuda")
        buf[:M, :K] = d["A"].to(torch.bfloat16)
    return buf


@functools.lru_cache(maxsize=4)
def b_buffer(M, N, K, ops, ldb, ldb2, b2_first=False):
    """(allocation, B view, B2 view or None).  B has 8 readable rows more than it has columns of the product; they hold NaN."""
    d = problem(M, N, K, ops)
    if ops == OPS_BF16:
        buf = torch.full((N + 8, ldb), NAN, dtype=torch.bfloat16, device="cuda")
        buf[:N, :K] = d["W"].to(torch.bfloat16)
        return buf, buf, None
    n8 = d["n_fp8"]
    if ops != OPS_TAIL:
        buf = torch.full((n8 + 8, ldb), FP8_NAN, dtype=torch.uint8, device="cuda")
        buf[:n8, :K] = d["codes"]
        return buf, buf, None
    # the bf16 tail lies behind B in ONE allocation (it is addressed through B's buffer descriptor)
    cbytes, tbytes = (n8 + 8) * ldb, (TAIL_ROWS + 8) * ldb2 * 2
    cbytes_al = (cbytes + 255) // 256 * 256
    raw = torch.full((cbytes_al + tbytes + 256,), FP8_NAN, dtype=torch.uint8, device="cuda")
    c_off, t_off = (tbytes + 255) // 256 * 256 if b2_first else 0, 0 if b2_first else cbytes_al
    codes = raw[c_off:c_off + cbytes].view(n8 + 8, ldb)
    codes[:n8, :K] = d["codes"]
    tail = raw[t_off:t_off + tbytes].view(torch.bfloat16).view(TAIL_ROWS + 8, ldb2)
    tail.fill_(NAN)
    tail[:TAIL_ROWS, :K] = d["W"][n8:].to(torch.bfloat16)
    return raw, codes, tail


# ------------------------------------------------------------------------------------------------ one launch
def launch(lib, ws, c, fields=None, b2_first=False, workspace=True):
    """fills the argument struct of case c and launches; returns (rc, {slot: (buffer, rows, width)}).  `fields` overrides
    struct members afterwards (the refusals)."""
    M, N, K, epi, ops = c.M, c.N, c.K, c.epi, c.ops
    d, geo, p = problem(M, N, K, ops), geometry(c.epi, M, N, ops), pitches(c)
    a = PevitGemmExArgs()
    a.set_tune(**VARIANTS[c.variant][1])
    A = a_buffer(M, N, K, ops, p.lda)
    raw, B, B2 = b_buffer(M, N, K, ops, p.ldb, p.ldb2, b2_first)
    a.epilogue, a.M, a.N, a.K = epi, M, N, K
    a.A, a.lda, a.B, a.ldb, a.b_rows = A.data_ptr(), p.lda, B.data_ptr(), p.ldb, B.shape[0]
    a.b_fp8, a.a_fp8 = int(ops != OPS_BF16), int(ops == OPS_FP8A)
    if B2 is not None:
        a.B2, a.ldb2, a.b2_rows, a.n_fp8 = B2.data_ptr(), p.ldb2, B2.shape[0], d["n_fp8"]
    if ops != OPS_BF16:
        a.bscale = d["bscale"].data_ptr()
    a.bias = d["bias"].data_ptr()
    if epi == DGELU:
        a.oscale = d["oscale"].data_ptr()
    if workspace:
        a.sk_slab, a.sk_flag, a.sk_slots = ws.slab.data_ptr(), ws.flag.data_ptr(), ws.slots
    outs, keep = {}, [A, raw]
    f32, bf16 = torch.float32, torch.bfloat16
    # operands the epilogue reads
    if epi in (BIAS_RESID, KEEP):
        if c.inplace:                                         # out_f32 IS the residual buffer (how the step calls it)
            r = torch.full((M + 1, p.ldr), SENT, dtype=f32, device="cuda")
            r[:M, :N] = d["resid"]
            outs["outf"] = (r, M, N)
            a.out_f32, a.ldo = r.data_ptr(), p.ldr
        else:
            r = padded_input(d["resid"], p.ldr, f32)
        a.resid, a.ldr = r.data_ptr(), p.ldr
        keep.append(r)
    if epi == PATCH:
        r = padded_input(d["pos"][:geo["Ntok"]], p.ldr, f32)
        a.resid, a.ldr, a.tokens = r.data_ptr(), p.ldr, geo["Ntok"]
        keep.append(r)
    if epi in (DGELU, DRELU, DGELUNEW):
        x = padded_input(d["aux"], p.ldaux, bf16)
        a.aux_bf16, a.ldaux = x.data_ptr(), p.ldaux
        keep.append(x)
    # outputs
    if epi == QKV:
        E, H, Ntok = geo["E"], geo["H"], geo["Ntok"]
        a.E, a.H, a.tokens, a.head_stride = E, H, Ntok, M * E
        outs["outb"] = (guarded(1, 3 * M * E, bf16, 3 * M * E + 64), 1, 3 * M * E)
        outs["outf"] = (guarded(M, N - 3 * E, f32, p.ldo), M, N - 3 * E)
    elif epi in LINEAR_F32 and "outf" not in outs:
        rows = geo["Bt"] * geo["Ntok"] if epi == PATCH else M
        outs["outf"] = (guarded(rows, N, f32, p.ldo), rows, N)
        if epi == PATCH:                                      # row 0 of every image belongs to the guard
            outs["outf"][0][:rows].view(geo["Bt"], geo["Ntok"], p.ldo)[:, 0] = SENT
    if epi == KEEP:
        outs["outf2"] = (guarded(M, N, f32, p.ldo2), M, N)
    if epi in (BIAS_GELU, BIAS_GELUNEW, DGELU, DRELU, DGELUNEW) or (epi in LINEAR_BF16 and epi != QKV):
        outs["outb"] = (guarded(M, N, bf16, p.ldob), M, N)
    if epi in (BIAS_GELU, BIAS_GELUNEW, GELU_ONLY):
        outs["outb2"] = (guarded(M, N, bf16, p.ldob2), M, N)
    for slot, member, ld in (("outf", "out_f32", "ldo"), ("outf2", "out_f32_2", "ldo2"), ("outb", "out_bf16", "ldob"),
                             ("outb2", "out2_bf16", "ldob2")):
        if slot in outs and not (slot == "outf" and c.inplace):
            setattr(a, member, outs[slot][0].data_ptr())
            setattr(a, ld, outs[slot][0].stride(0))
    for k, v in (fields or {}).items():
        setattr(a, k, v)
    rc = lib.pevit_op_gemm_ex(S(), C.byref(a))
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                 # a device fault is sticky: nothing more is started on the GPU
        pytest.exit(f"GPU error after {case_id(c)}: {e}", returncode=3)
    del keep
    return rc, outs


def payload(outs, slot):
    t, rows, width = outs[slot]
    return t[:rows, :width]


def untouched(c, outs):
    """no output of a refused launch was written"""
    for slot, (t, rows, width) in outs.items():
        if not guard_intact(t, rows, width):
            return False
        if slot == "outf" and c.inplace:
            continue
        pl = t[:rows, :width]
        if not bool((torch.isnan(pl) | (pl == SENT)).all()):
            return False
    return True


def check(lib, ws, c, outs):
    """guards, bit equality of the linear outputs, the gate of the nonlinear ones"""
    epi = c.epi
    d, geo = problem(c.M, c.N, c.K, c.ops), geometry(epi, c.M, c.N, c.ops)
    ref = reference(epi, d, d["acc"], geo)
    for slot, (t, rows, width) in outs.items():
        assert guard_intact(t, rows, width), f"{slot}: a store outside the payload"
    for slot in LINEAR_F32.get(epi, ()) + LINEAR_BF16.get(epi, ()):
        exp = ref[slot].float()
        exp = torch.where(torch.isnan(exp), torch.full_like(exp, SENT), exp)       # PATCH_EMBED: the rows it must leave alone
        if slot in LINEAR_BF16.get(epi, ()):
            exp = exp.to(torch.bfloat16)
        got = payload(outs, slot).reshape(exp.shape)
        if not same_bits(got, exp):
            bad = bits(got) != bits(exp)
            idx = bad.nonzero()[0].tolist()
            raise AssertionError(f"{slot}: {int(bad.sum())} of {bad.numel()} elements differ from the float64 reference, first at "
                                 f"{idx}: got {float(got[tuple(idx)])!r}, expected {float(exp[tuple(idx)])!r}")
    err = None
    if epi in (BIAS_GELU, BIAS_GELUNEW, GELU_ONLY):
        if epi == GELU_ONLY:                                   # the same g as BIAS_GELU, from the h that one stores
            rc, sib = launch(lib, ws, c._replace(epi=BIAS_GELU))
            assert rc == 0, lib.pevit_last_error().decode()
            assert same_bits(payload(outs, "outb2"), payload(sib, "outb2")), "GELU_ONLY's g differs from BIAS_GELU's"
            h = payload(sib, "outb")
        else:
            h = payload(outs, "outb")
        g = payload(outs, "outb2")
        assert torch.isfinite(g.float()).all()
        err = max_rel(g, activation(epi, h.double()))
    elif epi in (DGELU, DRELU, DGELUNEW):
        got = payload(outs, "outb")
        assert torch.isfinite(got.float()).all()
        err = max_rel(got, ref["outb"])
    if err is not None:
        MEASURED[epi] = max(MEASURED.get(epi, 0.0), err)
        assert err < NONLINEAR_GATE, f"{EPI_NAMES[epi]}: {err:.3e} of the largest magnitude"


def flags_clear(ws):
    return not bool(ws.flag.any())


def run_existing(lib, ws, c):
    rc, outs = launch(lib, ws, c)
    assert rc == 0, lib.pevit_last_error().decode()
    took = lib.pevit_debug_last_gemm_path()
    assert took == path_of(c), f"the planner took family {took}, the case names {path_of(c)}"
    assert flags_clear(ws), f"flag words / error word left set: {ws.flag.nonzero().flatten().tolist()[:8]} (error word at {ws.slots})"
    check(lib, ws, c, outs)
    return outs


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_gemm_form(lib, ws, c):
    first = run_existing(lib, ws, c)
    if path_of(c) in (5, 7):                                  # hand-offs between workgroups: three launches, identical bits
        for _ in range(2):
            again = run_existing(lib, ws, c)
            for slot in first:
                assert same_bits(first[slot][0], again[slot][0]), f"{slot} changed between launches"


@pytest.mark.parametrize("c", ABSENT, ids=case_id)
def test_absent_combination(lib, ws, c):
    before = lib.pevit_debug_last_gemm_path()
    rc, outs = launch(lib, ws, c)
    if absent_outcome(path_of(c), c.epi, c.ops) == "refused":
        assert rc == -1
        msg = lib.pevit_last_error().decode()
        want = ("no kernel with a bf16 tail" if c.ops == OPS_TAIL else "has no fp8-weight form" if c.ops == OPS_FP8B
                else "has no fp8 x fp8 form")
        assert want in msg, msg
        assert untouched(c, outs) and lib.pevit_debug_last_gemm_path() == before and flags_clear(ws)
    else:
        assert rc == 0, lib.pevit_last_error().decode()
        assert lib.pevit_debug_last_gemm_path() != path_of(c)
        assert flags_clear(ws)
        check(lib, ws, c, outs)


_BASE = Case("tile-cfg0", F32, OPS_BF16, 333, 264, 192, False)
_BASE8 = Case("tile-cfg0", F32, OPS_FP8B, 333, 264, 256, False)
_TAIL = Case("stag-cfg4", QKV, OPS_TAIL, 330, 832, 256, False)
REFUSALS = {
    "K-not-multiple-of-64": (_BASE, dict(K=96), "K=96 must be a positive multiple of 64"),
    "N-not-multiple-of-8": (_BASE, dict(N=260), "N=260 must be a multiple of 8"),
    "bad-lda": (_BASE, dict(lda=192 + 4), "lda/ldb"),
    "bad-ldb": (_BASE, dict(ldb=192 + 12), "lda/ldb"),
    "fp8-ldb-not-multiple-of-16": (_BASE8, dict(ldb=256 + 8), "lda/ldb"),
    "fp8-K-not-multiple-of-128": (_BASE8, dict(K=192), "multiple of 128"),
    "epilogue-15": (_BASE, dict(epilogue=15), "unknown epilogue 15"),
    "epilogue-minus-1": (_BASE, dict(epilogue=-1), "unknown epilogue -1"),
    "tail-on-cfg0": (_TAIL._replace(variant="tile-cfg0"), {}, "bf16 tail"),
    "tail-on-cfg3": (_TAIL._replace(variant="stag-cfg3"), {}, "bf16 tail"),
    "tail-n_fp8-not-multiple-of-256": (_TAIL, dict(n_fp8=640), "bf16 tail"),
    "tail-B2-in-front-of-B": (_TAIL, dict(), "bf16 tail"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_planner_refuses_before_any_launch(lib, ws, name):
    c, fields, words = REFUSALS[name]
    before = lib.pevit_debug_last_gemm_path()
    rc, outs = launch(lib, ws, c, fields, b2_first=name == "tail-B2-in-front-of-B")
    assert rc == -1
    assert words in lib.pevit_last_error().decode(), lib.pevit_last_error().decode()
    assert untouched(c, outs) and lib.pevit_debug_last_gemm_path() == before and flags_clear(ws)


def test_tail_kernel_exists_where_the_refusals_say_it_does_not(lib, ws):
    """the control of the tail refusals: the same launch without the fault succeeds (CASES holds it), so the refusals above are the
    planner's answer to the fault and not to the fixture"""
    assert _TAIL in CASES
    run_existing(lib, ws, _TAIL)


def test_families_without_a_workspace_are_not_taken(lib, ws):
    """no workspace: stream-K, the few-row kernel and the two-slice tile need one and are left out; the result is the same"""
    for c in (Case("streamk", F32, OPS_BF16, 300, 136, 2048, False), Case("fewrow-s0", F32, OPS_BF16, 37, 72, 1536, False),
              Case("kz2", F32, OPS_BF16, 2296, 1000, 2048, False)):
        rc, outs = launch(lib, ws, c, workspace=False)
        assert rc == 0, lib.pevit_last_error().decode()
        assert lib.pevit_debug_last_gemm_path() not in (5, 6, 7)
        check(lib, ws, c, outs)


def test_the_call_leaves_the_default_tune_alone(lib, ws):
    """a forced configuration in the struct's tune does not reach the plain entry point: it still takes its heuristic's family"""
    M, N, K = 37, 72, 1536
    d = problem(M, N, K, OPS_BF16)
    A, W = d["A"].to(torch.bfloat16).contiguous(), d["W"].to(torch.bfloat16).contiguous()

    def plain():
        out = torch.full((M, N), NAN, device="cuda")
        rc = lib.pevit_op_gemm(S(), F32, A.data_ptr(), K, W.data_ptr(), K, N, M, N, K, None, None, 0, out.data_ptr(), N, None, 0,
                               None, 0, None, 0, 0, 0, 0, 0)
        assert rc == 0, lib.pevit_last_error().decode()
        torch.cuda.synchronize()
        return lib.pevit_debug_last_gemm_path(), out

    path0, out0 = plain()
    run_existing(lib, ws, Case("tile-cfg2", F32, OPS_BF16, 333, 264, 192, False))
    path1, out1 = plain()
    assert path0 == path1 == 6 and same_bits(out0, out1) and same_bits(out0, d["acc"].float())


def test_zz_report_measured_deviations():
    """`pytest -s`: the figures of the module docstring"""
    print("\nlargest nonlinear deviation per epilogue: " + "  ".join(f"{EPI_NAMES[e]} {v:.2e}" for e, v in sorted(MEASURED.items())))
