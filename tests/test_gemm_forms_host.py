"""Host side of tests/test_gpu_gemm_forms.py (no GPU): the case table of the GEMM family, the operand generator, the float64
references of the fifteen epilogues, and the evidence that the comparison can see what it is meant to see.  No kernel is
launched: the last section calls the planner (csrc/gemm_plan.hip, pure host code) through pevit_debug_gemm_plan.

The family units of gemm.hip (gemm_tile.hip, gemm_stag8.hip, gemm_split.hip, gemm_streamk.hip, gemm_skinny.hip) instantiate kernels
from fifteen epilogues, seven kernel families (GemmPlan::path 1..7) and three operand forms (bf16 x
bf16, bf16 x fp8 B -- with or without a bf16 tail --, fp8 x fp8).  The GPU file launches every (family, epilogue, operand form)
combination that has an instantiation and compares it BIT FOR BIT with the float64 reference stated here.  That is possible because
the operands are small integers times powers of two:

    A          integers in [-2, 2] x 2^-2        exact in bf16 and in e4m3; the pre-activation covers the live range of the GELUs
    B          integers in [-2, 2]               (fp8 B: times a power-of-two channel scale 2^-3 .. 2^0, which the quantiser of
                                                 pevit_amd/fp8.py takes out again: the codes are +-128 / +-256)
    bias       integers in [-8, 8] x 2^-2
    residual, positional table   integers in [-64, 64]
    aux        integers in [-12, 12] x 2^-2      bf16-exact, covers the live range of the GELU derivatives
    oscale     powers of two 2^-2 .. 2^1

Every product, every partial sum and every epilogue sum is then exact in f32 (|acc| <= K < 2^24 / 2^5, everything a multiple of
2^-5), so the result does not depend on the order or the split of the summation: the k-split, phased, stream-K, few-row and
two-slice families must reproduce the same bits as the plain tiles.  An f32 output IS the float64 value; a bf16 output of a linear
epilogue is its round-to-nearest-even.  relu counts as linear here: max(x, 0) of an exact x is exact.  The nonlinear outputs -- g of
QuickGELU and gelu_new, the three derivative epilogues -- are compared (GPU file) with float64 evaluated on the kernel's own stored
bf16 h / on aux at the project's 1e-2 of the largest magnitude (tests/test_gpu_ops.py).

This file asserts, for every case of the table: float64 product == float32 product, max|acc| < 2^24, every operand stated as
bf16-exact is bf16-exact, the fp8 codes de-quantise to the integers bit for bit; that the table holds every combination the
statement `exists` admits and none twice; and the bite: for each epilogue the reference is mutated the way a subtly wrong kernel
would be wrong (one k-tile dropped, bias of column n + 1, residual / aux / positional row m + 1, PATCH_EMBED without its + 1, the
`which` and `h` indices of the head layout swapped, KEEP's outputs exchanged, the t columns taken with the bias) and must differ
from the true one -- the generated inputs are not degenerate for that fault.

The planner: the hand-written trait sets below equal epi_traits of the library for all fifteen epilogues; for every case of the table
plan_gemm at 256 CUs takes the family the case names, with the configuration, slice count, grid and band the variant and the shape
comments state; every absent combination is refused or falls to another family as absent_outcome says; and the plain-tile cases plan
without error at 304 and at 64 CUs within the residency slots of their configuration (the CU count is the only device fact the planner
is given).
"""
import collections
import ctypes as C
import functools
import os
import types

import pytest
import torch

from conftest import max_rel
from pevit_amd import _lib, fp8
from pevit_amd._lib import PevitGemmExArgs, PevitGemmPlanInfo

# ---------------------------------------------------------------------------------------------------- epilogues, operand forms
(QKV, BIAS_RESID, BIAS_GELU, DGELU, F32, BF16, BIAS_BF16, PATCH, BIAS_RELU, KEEP, BIAS_GELUNEW, DRELU, DGELUNEW, BIAS_F32,
 GELU_ONLY) = range(15)
EPI_NAMES = ("QKV", "BIAS_RESID", "BIAS_GELU", "DGELU", "F32", "BF16", "BIAS_BF16", "PATCH", "BIAS_RELU", "KEEP", "BIAS_GELUNEW",
             "DRELU", "DGELUNEW", "BIAS_F32", "GELU_ONLY")
ALL_EPIS = tuple(range(15))
OPS_BF16, OPS_FP8B, OPS_FP8A, OPS_TAIL = 0, 1, 2, 3        # TAIL: fp8 B with a bf16 tail (B2), gemm8_kernel<.., OPS = 1>
OPS_NAMES = ("bf16", "fp8b", "fp8xfp8", "fp8b+tail")
NONLINEAR_GATE = 1e-2                                       # tests/test_gpu_ops.py: bf16 outputs, relative to the largest magnitude

# gemm_plan.h epi_traits, restated: which families have an instantiation for an epilogue (checked against the library below)
FP8B_EPIS = frozenset((QKV, BIAS_RESID, BIAS_GELU, GELU_ONLY, DGELU, F32, BF16, BIAS_F32))
FP8A_EPIS = frozenset((QKV, BIAS_RESID, BIAS_GELU, GELU_ONLY, F32))
FEWROW_EPIS = frozenset((BIAS_RESID, F32, BF16, KEEP, BIAS_GELU, GELU_ONLY, DGELU))
SPLIT_EPIS = frozenset((BIAS_RESID, F32, BF16, KEEP, PATCH))
PATHS = (1, 2, 3, 4, 5, 6, 7)       # 1 tile, 2 staggered 8-wave, 3 k-split, 4 phased k-split, 5 stream-K, 6 few rows, 7 two K slices per tile
SPLIT_PATHS = (3, 4, 5, 7)


def exists(path, epi, ops):
    """do the family units of gemm.hip (FAMILY::launch) instantiate family `path` for this epilogue and operand form?"""
    if ops == OPS_FP8A:
        return path == 2 and epi in FP8A_EPIS            # always the 160x256 tile of the staggered kernel
    if ops == OPS_TAIL:
        return path == 2 and epi == QKV                  # ... on its 256-column tiles
    if ops == OPS_FP8B:
        return path in (1, 2) and epi in FP8B_EPIS
    if path in (1, 2):
        return True
    return epi in (FEWROW_EPIS if path == 6 else SPLIT_EPIS)


def in_domain(path, ops):
    """the bf16 tail is a property of one product (N = 3E + 64 on a forced tile configuration): stated for paths 1 and 2 only"""
    return ops != OPS_TAIL or path in (1, 2)


def absent_outcome(path, epi, ops):
    """what asking for an absent combination gives: the planner's refusal, or another family"""
    assert not exists(path, epi, ops)
    if ops == OPS_TAIL or (ops == OPS_FP8B and epi not in FP8B_EPIS) or (ops == OPS_FP8A and epi not in FP8A_EPIS):
        return "refused"
    return "fallback"


# ---------------------------------------------------------------------------------------------------- family variants and the table
# name -> (path, tune).  A forced `config` switches the few-row, k-split and stream-K families off (plan_tiles).
VARIANTS = {}
for _c in (0, 1, 2, 6, 7, 8):
    VARIANTS[f"tile-cfg{_c}"] = (1, dict(config=_c))
for _c in (3, 4, 5):
    VARIANTS[f"tile-cfg{_c}"] = (1, dict(config=_c, stagger=0))          # the 8-wave tiles on gemm_kernel
for _c in (4, 5, 9):
    VARIANTS[f"stag-cfg{_c}"] = (2, dict(config=_c))
VARIANTS["stag-cfg3"] = (2, dict(config=3, stagger=2))                   # 256x128, two k-steps per phase
VARIANTS["ksplit-s0"] = (3, dict(ksplit_stagger=0, ksplit_mink=64))
VARIANTS["ksplit-s1"] = (3, dict(ksplit_stagger=1, ksplit_mink=64))
VARIANTS["kphase-nl8"] = (4, dict(ksplit_stagger=2, kphase_nl=8, ksplit_mink=64))
VARIANTS["kphase-nl2"] = (4, dict(ksplit_stagger=2, kphase_nl=2, ksplit_mink=64))
VARIANTS["streamk"] = (5, dict())
for _s in (0, 1, 3, 6):
    VARIANTS[f"fewrow-s{_s}"] = (6, dict(skinny_slices=_s))              # 0 = the automatic rule (two slices at 24 k-tiles)
VARIANTS["kz2"] = (7, dict(kz2=1))
REPRESENTATIVE = {1: "tile-cfg0", 2: "stag-cfg9", 3: "ksplit-s1", 4: "kphase-nl8", 5: "streamk", 6: "fewrow-s0", 7: "kz2"}

Case = collections.namedtuple("Case", "variant epi ops M N K inplace")


def case_id(c):
    return f"{c.variant}-{EPI_NAMES[c.epi]}-{OPS_NAMES[c.ops]}-{c.M}x{c.N}x{c.K}" + ("-inplace" if c.inplace else "")


def path_of(c):
    return VARIANTS[c.variant][0]


def tune_of(c):
    return VARIANTS[c.variant][1]


# Shapes (256 CUs).  333 is ragged for every tile height, 264 = 256 + one eight-column remainder; the QKV product has E = 128, H = 2,
# T = 30 x 11 tokens, N = 3E + 64 = 448: the 3E boundary lies inside a 256-wide tile.
SHAPE, SHAPE_QKV = (333, 264), (330, 448)
TAIL_SHAPE, TAIL_NFP8 = (330, 832), 768                      # E = 256, H = 4, n_fp8 = 3E, the 64 tail columns in a tile of their own
# one tile per CU on (wm x 32) x 128 tiles (use_ksplit): 3828 -> 24 x 8 = 192 tiles of 160x128 (xcd_band 3), 3971 -> 25 x 8 = 200
# (25 m-tiles do not split over 8 XCDs: xcd_band 0), 2296 -> 24 x 8 = 192 tiles of 96x128 where 160x128 gives 120
SPLIT_SHAPES = ((3828, 1000, (64, 128, 192, 320)), (2296, 1000, (64, 128, 192, 320)), (3971, 1000, (128,)))
SPLIT_CASE_EPIS = (BIAS_RESID, F32, BF16, PATCH, KEEP)
KZ2_SHAPE, STREAMK_SHAPE, FEWROW_SHAPE = (2296, 1000), (300, 136), (37, 72)
LONG_KS = (2048, 2112)              # 2112: an odd number of k-tiles (33); stream-K share 18 straddles tile boundaries, grid 11 -> 16
FEWROW_K = 1536
FEWROW_CASE_EPIS = (BIAS_RESID, F32, BF16, KEEP, BIAS_GELU, GELU_ONLY, DGELU)
MANY_TILES = (5281, 2056, 128)      # 160x256: 34 x 9 = 306 tiles on 256 workgroups, the persistent walk takes a second tile


def _split_epis():
    return [(e, False) for e in SPLIT_CASE_EPIS] + [(BIAS_RESID, True), (KEEP, True)]       # ... also in place on the residual buffer


def _build_cases():
    cases = []
    for v, (path, _) in VARIANTS.items():
        if path in (1, 2):
            for K in (192, 64):
                for e in ALL_EPIS:
                    M, N = SHAPE_QKV if e == QKV else SHAPE
                    cases.append(Case(v, e, OPS_BF16, M, N, K, False))
    for e in (BIAS_RESID, BF16):
        cases.append(Case("stag-cfg9", e, OPS_BF16, *MANY_TILES, False))
    for v in ("ksplit-s0", "ksplit-s1", "kphase-nl8", "kphase-nl2"):
        for M, N, Ks in SPLIT_SHAPES:
            for K in Ks:
                cases += [Case(v, e, OPS_BF16, M, N, K, ip) for e, ip in _split_epis()]
    for K in LONG_KS:
        cases += [Case("kz2", e, OPS_BF16, *KZ2_SHAPE, K, ip) for e, ip in _split_epis()]
        cases += [Case("streamk", e, OPS_BF16, *STREAMK_SHAPE, K, ip) for e, ip in _split_epis()]
    for s in (0, 1, 3, 6):
        cases += [Case(f"fewrow-s{s}", e, OPS_BF16, *FEWROW_SHAPE, FEWROW_K, False) for e in FEWROW_CASE_EPIS]
    for v in ("tile-cfg0", "tile-cfg1", "stag-cfg4", "stag-cfg5", "stag-cfg9"):
        for e in sorted(FP8B_EPIS):
            M, N = SHAPE_QKV if e == QKV else SHAPE
            cases.append(Case(v, e, OPS_FP8B, M, N, 256, False))
    for e in sorted(FP8A_EPIS):
        M, N = SHAPE_QKV if e == QKV else SHAPE
        cases.append(Case("stag-cfg9", e, OPS_FP8A, M, N, 256, False))
    for v in ("stag-cfg4", "stag-cfg5", "stag-cfg9"):
        cases.append(Case(v, QKV, OPS_TAIL, *TAIL_SHAPE, 256, False))
    return cases


CASES = _build_cases()


def absent_shape(path, epi):
    """a shape on which the tune of REPRESENTATIVE[path] would take `path` if the combination existed (QKV: N = 3E + 64)"""
    q = epi == QKV
    return {1: (*(SHAPE_QKV if q else SHAPE), 256), 2: (*(SHAPE_QKV if q else SHAPE), 256),
            3: (3828, 1024 if q else 1000, 128), 4: (3828, 1024 if q else 1000, 128),
            5: (300, 256 if q else 136, 2048), 6: (33 if q else 37, 448 if q else 72, FEWROW_K),
            7: (2296, 1024 if q else 1000, 2048)}[path]


def _build_absent():
    out = []
    for path in PATHS:
        for ops in (OPS_BF16, OPS_FP8B, OPS_FP8A, OPS_TAIL):
            for e in ALL_EPIS:
                if in_domain(path, ops) and not exists(path, e, ops):
                    v = REPRESENTATIVE[path] if not (path == 2 and ops == OPS_TAIL) else "stag-cfg4"
                    shape = (*TAIL_SHAPE, 256) if ops == OPS_TAIL else absent_shape(path, e)
                    out.append(Case(v, e, ops, *shape, False))
    return out


ABSENT = _build_absent()


# ---------------------------------------------------------------------------------------------------- geometry of the remapping epilogues
def _divisor(M, first=7):
    return next(d for d in range(first, M + 1) if M % d == 0)


def geometry(epi, M, N, ops=OPS_BF16):
    """E, H, Ntok of the head-layout epilogue (N = 3E + 64) and Ntok of the patch embedding (M = Bt x (Ntok - 1))"""
    if epi == QKV:
        E = (N - 64) // 3
        assert 3 * E + 64 == N and E % 64 == 0, (M, N)
        Ntok = 11 if M % 11 == 0 else _divisor(M)
        return dict(E=E, H=E // 64, Ntok=Ntok, Bt=M // Ntok)
    if epi == PATCH:
        G2 = _divisor(M)                 # 333 = 37 x 9, 3828 = 348 x 11, 3971 = 361 x 11, 2296 = 328 x 7, 300 = 30 x 10, 37 = 1 x 37
        return dict(E=0, H=0, Ntok=G2 + 1, Bt=M // G2)
    return dict(E=0, H=0, Ntok=0, Bt=0)


# ---------------------------------------------------------------------------------------------------- pitches of one launch
TAIL_ROWS = 64                      # rows of the bf16 tail B2 (P_q^T | P_v^T)


def pitches(c):
    """row pitches of one launch: pairwise different, none equal to a width of the problem"""
    widths, taken, p = {c.N, c.K, 64}, set(), {}

    def take(name, base):
        v = base + 16
        while v in taken or v in widths:
            v += 16
        taken.add(v)
        p[name] = v

    if path_of(c) == 6:
        p["lda"] = 3 * c.K                       # the class-token rows of the step: every third row of a [3M][K] buffer
        taken.add(p["lda"])
    else:
        take("lda", c.K)
    take("ldb", c.K); take("ldb2", c.K)
    for name in ("ldr", "ldo", "ldo2", "ldob", "ldob2", "ldaux"):
        take(name, c.N)
    if c.epi == QKV:
        take("ldo", 64)
    assert len(set(p.values())) == len(p) and not set(p.values()) & widths
    return types.SimpleNamespace(**p)


# ---------------------------------------------------------------------------------------------------- operands
def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def kpermuted(codes):
    """codes [rows][K] in the storage order of csrc/fp8.hip: input channel k sits at kperm(k)"""
    out = torch.empty_like(codes)
    out[:, fp8.kperm(codes.shape[1])] = codes
    return out


@functools.lru_cache(maxsize=4)
def operands(M, N, K, ops):
    """CPU tensors of one problem, never modified: A (M,K) and W (N,K) = what the kernel's B operand stands for, as f32 VALUES; the
    epilogue operands; for the fp8 forms the k-permuted codes and the channel scales the kernel is given"""
    g = torch.Generator(device="cpu").manual_seed(1000003 * M + 1009 * N + K)
    o = dict(M=M, N=N, K=K, ops=ops)
    o["A"] = _ints(g, (M, K), -2, 2) * 0.25
    b_int = _ints(g, (N, K), -2, 2)
    o["bias"] = _ints(g, (N,), -8, 8) * 0.25
    o["resid"] = _ints(g, (M, N), -64, 64)
    o["aux"] = _ints(g, (M, N), -12, 12) * 0.25
    o["oscale"] = torch.ldexp(torch.ones(N), _ints(g, (N,), -2, 1).int())
    chan = torch.ldexp(torch.ones(N), _ints(g, (N,), -3, 0).int())
    o["pos"] = _ints(g, (M + 1, N), -64, 64)                  # the positional table: its first Ntok rows are used
    if ops == OPS_BF16:
        o["W"] = b_int
    else:
        n8 = TAIL_NFP8 if ops == OPS_TAIL else N
        W = b_int * chan[:, None]
        W[n8:] = b_int[n8:]                                   # the bf16 tail carries no channel scale
        codes, scales = fp8.quantize_rows(W[:n8])
        o["W"], o["n_fp8"], o["codes_plain"], o["codes"] = W, n8, codes, kpermuted(codes)
        o["bscale"] = torch.full((N,), float("nan"))          # ... and the kernel must not read one for it
        o["bscale"][:n8] = scales
    if ops == OPS_FP8A:
        o["acodes_plain"] = o["A"].to(torch.float8_e4m3fn).view(torch.uint8)
        o["acodes"] = kpermuted(o["acodes_plain"])
    return o


def accumulate(o):
    """the exact product, float64"""
    return o["A"].double() @ o["W"].double().T


def _bf16_exact(t):
    return torch.equal(t.to(torch.bfloat16).to(t.dtype), t)


# ---------------------------------------------------------------------------------------------------- references
def head_layout(x, Bt, Ntok, H, swap=False):
    """(Bt*Ntok, 3*H*64) rows -> (which, b*H + h, n, d)"""
    x = x.reshape(Bt, Ntok, 3, H, 64)
    if swap:                                                  # the fault: column = (h, which, d) instead of (which, h, d)
        x = x.reshape(Bt, Ntok, H, 3, 64).permute(0, 1, 3, 2, 4)
    return x.permute(2, 0, 3, 1, 4).reshape(3, Bt * H, Ntok, 64)


def quick_gelu(h):
    return h * torch.sigmoid(1.702 * h)


def quick_gelu_grad(h):
    s = torch.sigmoid(1.702 * h)
    return s * (1 + 1.702 * h * (1 - s))


_C = 0.7978845608028654


def gelu_new(x):
    return 0.5 * x * (1 + torch.tanh(_C * (x + 0.044715 * x ** 3)))


def gelu_new_grad(x):
    th = torch.tanh(_C * (x + 0.044715 * x ** 3))
    return 0.5 * (1 + th) + 0.5 * x * (1 - th * th) * _C * (1 + 3 * 0.044715 * x * x)


LINEAR_F32 = {QKV: ("outf",), BIAS_RESID: ("outf",), F32: ("outf",), PATCH: ("outf",), KEEP: ("outf", "outf2"), BIAS_F32: ("outf",)}
LINEAR_BF16 = {QKV: ("outb",), BIAS_GELU: ("outb",), BF16: ("outb",), BIAS_BF16: ("outb",), BIAS_RELU: ("outb",), BIAS_GELUNEW: ("outb",)}
NONLINEAR = {BIAS_GELU: "outb2", GELU_ONLY: "outb2", BIAS_GELUNEW: "outb2", DGELU: "outb", DRELU: "outb", DGELUNEW: "outb"}


def reference(epi, o, acc, geo, mut=None):
    """float64 expected outputs {slot: tensor} of the LINEAR outputs (f32 slots hold the value itself, bf16 slots the value to be
    rounded to nearest even) and, for the derivative epilogues, of the nonlinear one.  o: operands() on any device; acc: accumulate(o).
    mut: one of MUTATIONS -- the reference of a kernel with that fault."""
    bias, resid, aux, pos = o["bias"].double(), o["resid"].double(), o["aux"].double(), o["pos"].double()
    if mut == "k_tile":
        acc = acc - o["A"][:, -64:].double() @ o["W"][:, -64:].double().T
    if mut == "bias_next":
        bias = bias.roll(-1)
    if mut == "row_next":
        resid, aux, pos = resid.roll(-1, 0), aux.roll(-1, 0), pos.roll(-1, 0)
    M, N = acc.shape
    if epi == QKV:
        E3 = 3 * geo["E"]
        t = acc[:, E3:] + (bias[E3:] if mut == "t_bias" else 0)
        return dict(outb=head_layout(acc[:, :E3] + bias[:E3], geo["Bt"], geo["Ntok"], geo["H"], swap=mut == "which_h"), outf=t)
    if epi == BIAS_RESID:
        return dict(outf=acc + bias + resid)
    if epi in (BIAS_GELU, GELU_ONLY, BIAS_GELUNEW, BIAS_BF16):
        return dict(outb=acc + bias)                          # GELU_ONLY does not store it: its g is held to BIAS_GELU's
    if epi == DGELU:
        return dict(outb=acc * quick_gelu_grad(aux) * o["oscale"].double())
    if epi == DRELU:
        return dict(outb=acc * (aux > 0))
    if epi == DGELUNEW:
        return dict(outb=acc * gelu_new_grad(aux))
    if epi == F32:
        return dict(outf=acc)
    if epi == BF16:
        return dict(outb=acc)
    if epi == BIAS_F32:
        return dict(outf=acc + bias)
    if epi == BIAS_RELU:
        return dict(outb=(acc + bias).clamp_min(0))
    if epi == KEEP:
        a, b = acc + bias + resid, acc + bias
        return dict(outf=b, outf2=a) if mut == "keep_swapped" else dict(outf=a, outf2=b)
    assert epi == PATCH
    Ntok, Bt = geo["Ntok"], geo["Bt"]
    G2, off = Ntok - 1, 0 if mut == "no_plus_one" else 1
    out = torch.full((Bt, Ntok, N), float("nan"), dtype=torch.float64, device=acc.device)      # NaN = a row the kernel does not write
    out[:, off:off + G2] = acc.view(Bt, G2, N) + pos[off:off + G2]
    return dict(outf=out.view(Bt * Ntok, N))


def activation(epi, h):
    """g of the stored pre-activation h (float64)"""
    return gelu_new(h) if epi == BIAS_GELUNEW else quick_gelu(h)


HAS_BIAS = frozenset((QKV, BIAS_RESID, BIAS_GELU, GELU_ONLY, BIAS_BF16, BIAS_RELU, KEEP, BIAS_GELUNEW, BIAS_F32))
ROW_OPERAND = frozenset((BIAS_RESID, KEEP, PATCH, DGELU, DRELU, DGELUNEW))


def mutations(epi):
    m = ["k_tile"]
    if epi in HAS_BIAS:
        m.append("bias_next")
    if epi in ROW_OPERAND:
        m.append("row_next")
    m += {QKV: ["which_h", "t_bias"], KEEP: ["keep_swapped"], PATCH: ["no_plus_one"]}.get(epi, [])
    return m


def differs(epi, true, mutated):
    """would the GPU file's comparison tell the two references apart?  Linear slots: other bits; the derivative epilogues: beyond
    their gate"""
    if epi in (DGELU, DRELU, DGELUNEW):
        return max_rel(mutated["outb"], true["outb"]) > NONLINEAR_GATE
    out = False
    for slot in true:
        a, b = true[slot], mutated[slot]
        if slot in LINEAR_BF16.get(epi, ()) or epi == GELU_ONLY:
            a, b = a.float().to(torch.bfloat16), b.float().to(torch.bfloat16)
        both = ~(torch.isnan(a.float()) & torch.isnan(b.float()))
        out = out or not torch.equal(a[both], b[both]) or not torch.equal(torch.isnan(a.float()), torch.isnan(b.float()))
    return out


# ---------------------------------------------------------------------------------------------------- the tests
def problems():
    """the distinct (M, N, K, ops) of the table and of the absent combinations"""
    return sorted({(c.M, c.N, c.K, c.ops) for c in CASES + ABSENT})


def test_table_covers_the_statement_exactly_once():
    assert len(set(CASES)) == len(CASES), "a case twice"
    have = {(path_of(c), c.epi, c.ops) for c in CASES}
    want = {(p, e, o) for p in PATHS for e in ALL_EPIS for o in range(4) if in_domain(p, o) and exists(p, e, o)}
    assert have == want, (sorted(want - have), sorted(have - want))
    assert not any(exists(path_of(c), c.epi, c.ops) for c in ABSENT) and len(set(ABSENT)) == len(ABSENT)
    absent = {(path_of(c), c.epi, c.ops) for c in ABSENT}
    assert absent == {(p, e, o) for p in PATHS for e in ALL_EPIS for o in range(4) if in_domain(p, o) and not exists(p, e, o)}
    # every instantiation the issue names by family variant is a variant of the table
    assert {path_of(c) for c in CASES} == set(PATHS)
    per_path = collections.Counter(path_of(c) for c in CASES)
    print(f"\n{len(CASES)} cases ({dict(sorted(per_path.items()))} per family), {len(want)} (family, epilogue, operand form) "
          f"combinations, {len(ABSENT)} absent ones, {len(problems())} distinct problems")


def test_pitch_rules_and_geometry_of_every_case():
    for c in CASES + ABSENT:
        assert c.K % 64 == 0 and c.N % 8 == 0 and (c.ops == OPS_BF16 or c.K % 128 == 0), c
        if c.epi in (QKV, PATCH):
            geo = geometry(c.epi, c.M, c.N, c.ops)
            assert geo["Bt"] * (geo["Ntok"] - (c.epi == PATCH)) == c.M and geo["Bt"] >= 1 and geo["Ntok"] >= 2, c
        if c.inplace:
            assert c.epi in (BIAS_RESID, KEEP)
    # the QKV cases of the 256-wide tiles hold the 3E boundary inside a tile; the tail starts on a tile boundary
    assert 256 < 3 * geometry(QKV, *SHAPE_QKV)["E"] < 448 and TAIL_NFP8 % 256 == 0 and TAIL_NFP8 == 3 * geometry(QKV, *TAIL_SHAPE)["E"]


@pytest.mark.parametrize("M,N,K,ops", problems(), ids=lambda v: str(v))
def test_operands_are_exact(M, N, K, ops):
    o = operands(M, N, K, ops)
    acc64 = accumulate(o)
    acc32 = o["A"] @ o["W"].T
    assert torch.equal(acc32.double(), acc64), "the float32 product is not the float64 product"
    amax = float(acc64.abs().max())
    assert amax < 2 ** 24 and amax > 0
    for name in ("A", "W", "aux"):
        assert _bf16_exact(o[name]), name
    for name in ("bias", "resid", "pos", "oscale"):           # f32 operands: exact sums need short mantissas
        assert _bf16_exact(o[name]), name
    # every epilogue sum is exact in f32 as well
    full = acc64 + o["bias"].double() + o["resid"].double()
    assert torch.equal(full.float().double(), full)
    if ops != OPS_BF16:
        n8 = o["n_fp8"]
        deq = fp8.dequantize_rows(o["codes_plain"], o["bscale"][:n8])
        assert torch.equal(deq, o["W"][:n8]), "the de-quantised codes are not the integers"
        m, _ = torch.frexp(o["bscale"][:n8])
        assert torch.all(m == 0.5)                            # powers of two
        assert torch.equal(o["codes"][:, fp8.kperm(K)], o["codes_plain"])
        # the accumulator of the CODES (before the channel scale) is exact too
        cacc = o["A"].double() @ o["codes_plain"].view(torch.float8_e4m3fn).double().T
        assert float(cacc.abs().max()) < 2 ** 24 and torch.equal(cacc * o["bscale"][:n8].double(), acc64[:, :n8])
    if ops == OPS_FP8A:
        assert torch.equal(o["acodes_plain"].view(torch.float8_e4m3fn).float(), o["A"])
    print(f"\n({M}, {N}, {K}, {OPS_NAMES[ops]}): exact, max|acc| = {amax:g}", end="")


@functools.lru_cache(maxsize=2)
def _acc(M, N, K, ops):
    return accumulate(operands(M, N, K, ops))


def _bite_problems():
    return [(e, M, N, K, ops) for M, N, K, ops, e in sorted({(c.M, c.N, c.K, c.ops, c.epi) for c in CASES})]


@pytest.mark.parametrize("epi,M,N,K,ops", _bite_problems(), ids=lambda v: str(v))
def test_mutated_references_differ(epi, M, N, K, ops):
    """the bite: the inputs of this problem are not degenerate for any fault of the list (an all-zero k-tile, a symmetric bias...)"""
    o = operands(M, N, K, ops)
    acc = _acc(M, N, K, ops)
    geo = geometry(epi, M, N, ops)
    true = reference(epi, o, acc, geo)
    assert not differs(epi, true, reference(epi, o, acc, geo))
    for mut in mutations(epi):
        assert differs(epi, true, reference(epi, o, acc, geo, mut)), f"{EPI_NAMES[epi]}: the fault '{mut}' is invisible on these inputs"


def test_nonlinear_operands_cover_the_live_range():
    """the pre-activation and aux reach both tails and the curved middle of the GELUs (a gate relative to the largest magnitude
    needs large and small values in one tensor)"""
    o = operands(*SHAPE, 192, OPS_BF16)
    h = accumulate(o) + o["bias"].double()
    assert float(h.min()) < -3 and float(h.max()) > 3 and float(((h.abs() > 0.2) & (h.abs() < 1.5)).double().mean()) > 0.05
    assert float(o["aux"].min()) == -3 and float(o["aux"].max()) == 3


# ---------------------------------------------------------------------------------------------------- the planner itself, no GPU
# pevit_debug_gemm_plan runs plan_gemm (csrc/gemm_plan.hip) on the argument struct pevit_op_gemm_ex would launch.  The planner reads
# pointers only as set / unset and as the B2 - B distance, so the addresses are made up: B2 behind B at the distance b_buffer of
# the GPU file gives it, a workspace of sk_slots(256) slots, the pitches of pitches(c).
CUS = 256
WGS = {0: 2, 1: 3, 2: 4, 3: 1, 4: 1, 5: 1, 6: 3, 7: 2, 8: 2}      # gemm_plan.h kConfigs: workgroups per CU of a tile configuration
_A0, _B0, _WS0 = 0x10000000, 0x20000000, 0x40000000


def sk_slots(cus):
    return min(2 * cus, 1024) & ~7


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def plan_args(c):
    p = pitches(c)
    a = PevitGemmExArgs()
    a.set_tune(**tune_of(c))
    n8 = TAIL_NFP8 if c.ops == OPS_TAIL else c.N
    a.epilogue, a.M, a.N, a.K = c.epi, c.M, c.N, c.K
    a.A, a.lda, a.B, a.ldb, a.b_rows = _A0, p.lda, _B0, p.ldb, n8 + 8
    a.b_fp8, a.a_fp8 = int(c.ops != OPS_BF16), int(c.ops == OPS_FP8A)
    if c.ops == OPS_TAIL:                                        # the tail behind the codes, 256-byte aligned (b_buffer)
        a.B2, a.ldb2, a.b2_rows, a.n_fp8 = _B0 + ((n8 + 8) * p.ldb + 255) // 256 * 256, p.ldb2, TAIL_ROWS + 8, n8
    a.ldr, a.ldo, a.ldo2, a.ldob, a.ldob2, a.ldaux = p.ldr, p.ldo, p.ldo2, p.ldob, p.ldob2, p.ldaux
    slots = sk_slots(CUS)
    a.sk_flag, a.sk_slab, a.sk_slots = _WS0, _WS0 + (slots + 1) * 4, slots
    return a


def plan(lib, c, cus=CUS):
    """(rc, pevit_gemm_plan_info) of case c on a device of `cus` compute units"""
    a, info = plan_args(c), PevitGemmPlanInfo()
    rc = lib.pevit_debug_gemm_plan(C.byref(a), cus, C.byref(info))
    assert (rc == 0 and info.err == b"") or (rc == -1 and info.err and info.err == lib.pevit_last_error())
    return rc, info


def test_trait_sets_are_the_librarys(lib):
    for e in ALL_EPIS:
        want = int(e in FP8B_EPIS) | int(e in FP8A_EPIS) << 1 | int(e in FEWROW_EPIS) << 2 | int(e in SPLIT_EPIS) << 3
        assert lib.pevit_debug_gemm_epi_traits(e) == want, EPI_NAMES[e]
    assert lib.pevit_debug_gemm_epi_traits(-1) == -1 and lib.pevit_debug_gemm_epi_traits(len(ALL_EPIS)) == -1
    assert PATCH not in FEWROW_EPIS and KEEP in FEWROW_EPIS


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_planner_takes_the_named_family(lib, c):
    rc, pl = plan(lib, c)
    assert rc == 0, pl.err
    assert pl.path == path_of(c), f"the planner takes family {pl.path} at {CUS} CUs, the case names {path_of(c)}"
    kind, _, arg = c.variant.partition("-")
    if kind in ("stag", "tile"):
        assert pl.cfg == int(arg[3:])                                   # the forced configuration
    if kind == "kphase":
        assert pl.nl == int(arg[2:])
    if kind in ("ksplit", "kphase"):
        assert pl.wm == (3 if c.M == 2296 else 5)                       # SPLIT_SHAPES: 2296 rows take the 96x128 tile
        assert pl.band == {3828: 3, 3971: 0}.get(c.M, pl.band)          # ... and the XCD-aligned bands stated there
    if kind == "ksplit":
        assert pl.stag == int(arg == "s1" or pl.wm == 3)                # 96x128 is always staggered
    if kind == "fewrow":
        assert c.K == FEWROW_K and pl.nslices == (int(arg[1:]) or 2)    # s0: the automatic rule, two slices at 24 k-tiles
    if (c.M, c.N, c.K) == MANY_TILES:
        assert (pl.tiles, pl.grid) == (306, 256)                        # the persistent walk takes a second tile
    if kind == "streamk" and c.K == 2112:
        assert (pl.sk_share, pl.grid) == (18, 16)                       # LONG_KS


@pytest.mark.parametrize("c", ABSENT, ids=case_id)
def test_planner_on_absent_combinations(lib, c):
    rc, pl = plan(lib, c)
    if absent_outcome(path_of(c), c.epi, c.ops) == "refused":
        assert rc == -1 and pl.err
    else:
        assert rc == 0 and pl.path != path_of(c)


def test_cus_is_the_only_device_fact_the_planner_uses(lib):
    """the plain-tile cases plan on any device: no error, and never more workgroups than the residency slots of the configuration"""
    n = 0
    for c in CASES:
        if c.variant.startswith("tile-"):
            for cus in (304, 64):
                rc, pl = plan(lib, c, cus)
                assert rc == 0 and pl.path == 1 and 0 < pl.grid <= WGS[pl.cfg] * cus, (case_id(c), cus, pl.grid)
                n += 1
    assert n >= 2 * 9 * len(ALL_EPIS)
