"""Host side of tests/test_gpu_kernel_forms.py (no GPU): the inputs of the attention token-count sweep, its float64 reference, and
the evidence that the sweep's gates can see what they are meant to see.

The sweep runs the attention kernels at token counts N where no tower fixture runs them (the two runtime-N forward instances, the
shared last tile of the backward kernel, the family boundaries).  Its gates are the ones of tests/test_gpu_ops.py -- out max-rel
1.5e-2, |lse - ref| 2e-2, gradient rel-L2 2e-2 -- and they are whole-tensor figures: one key too many or too few among 65..288 is
one column of the score matrix.  The sweep therefore doubles the LAST token's k, v and dO rows (exact in bf16), which puts a large
share of every row's probability mass and of the gradient on the one key an off-by-one mask gets wrong: with them, a last key
counted twice moves every checked quantity by at least 4x its gate (smallest: dV, 8.2e-2 at N = 273), a dropped one by 20x.

This file states, on the CPU and with the kernel nowhere in sight:

  * the float64 reference of the core and of its gradients on bf16 operands, with a weight on the last key (1 = the attention
    core; 2 = the last key counted twice; 0 = the last key dropped);
  * an emulation of the kernels' rounding points in float64 arithmetic: the probabilities are rounded to bf16 BEFORE the row sum
    and the P.V product (attention.hip: the normaliser is the sum of what the product sees), out is stored in bf16, lse is
    m + log(that sum); the backward pass reads the stored bf16 out for delta = sum(dO * out), recomputes P = exp(S - lse), rounds
    dS = P (dP - delta) and P to bf16 before the three gradient products and stores the gradients in bf16;
  * the floor: that emulation against the float64 reference.  It must stay below every gate (it does by 4x or more);
  * the bite: both off-by-one variants against the float64 reference.  Each must exceed EVERY gate -- out, lse, dQ, dK, dV -- at
    every N of the sweep.

The emulation is the reference here, never the kernel.  `pytest -s` prints the floors; the GPU file's docstring records them.
"""
import pytest
import torch

from conftest import max_rel, rel_err

# token counts of the sweep -> the kernel instance each lands in (it follows from N alone, attention.hip pevit_launch_attn_fwd / _bwd):
#   forward : 65, 128, 129, 144, 145, 224 -> runtime-N instance <KT32 = 7, 4 waves> (65..224, except the compile-time 197)
#             225, 226, 272, 273, 288     -> runtime-N instance <KT32 = 9, 8 waves> (225..288, except the compile-time 257)
#   backward: 65 .. 224 -> <KT32 = 7, 8 waves, padded LDS rows>; its last 16-row tile is shared between the waves when
#             ntile % 8 == 1 and ntile > 8, i.e. N in [129, 144]: 129 and 144 (9 tiles) enter it, 128 (8) and 145 (10) do not
#             225 .. 288 -> <KT32 = 9, 16 waves, swizzled LDS rows>; shared last tile for N in [257, 272]: 272 (17 tiles) enters it,
#             273 (18 tiles) does not; 288 = the cap, 224 | 225 the family boundary, 64 | 65 the boundary to the all-in-LDS kernel
SWEEP_N = (65, 128, 129, 144, 145, 224, 225, 226, 272, 273, 288)
SWEEP_BT, SWEEP_H = 2, 3           # several (b, h) workgroups per launch, an odd head count: the b*N / h*64 addressing
OUT_GATE, LSE_GATE, GRAD_GATE = 1.5e-2, 2e-2, 2e-2       # tests/test_gpu_ops.py test_attention_fwd_bwd


def _rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


def sweep_inputs(N, Bt=SWEEP_BT, H=SWEEP_H, double_last=True):
    """q, k, v (Bt*H, N, 64) and dO (Bt*N, H*64) in bf16 on the CPU: the recipe of test_attention_fwd_bwd, with the last token's
    k, v and dO rows doubled"""
    E = H * 64
    q = _rnd(Bt * H, N, 64, seed=1, scale=0.35)
    k = _rnd(Bt * H, N, 64, seed=2)
    v = _rnd(Bt * H, N, 64, seed=3)
    do = _rnd(Bt * N, E, seed=4)
    if double_last:
        k[:, N - 1] *= 2
        v[:, N - 1] *= 2
        do.view(Bt, N, E)[:, N - 1] *= 2
    return q, k, v, do


def heads_of(rows, Bt, H, N):
    """(Bt*N, H*64) row layout -> (Bt*H, N, 64) head layout"""
    return rows.reshape(Bt, N, H, 64).permute(0, 2, 1, 3).reshape(Bt * H, N, 64)


def rows_of(heads, Bt, H, N):
    """(Bt*H, N, 64) head layout -> (Bt*N, H*64) row layout"""
    return heads.reshape(Bt, H, N, 64).permute(0, 2, 1, 3).reshape(Bt * N, H * 64)


def attn_ref64(q, k, v, do_heads, last_key_weight=1.0):
    """float64 attention core and its gradients, everything in the head layout: out, lse, dq, dk, dv.
    The last key enters the softmax with `last_key_weight` (P_ij = w_j e^S_ij / sum_j w_j e^S_ij): 1 is the attention core,
    2 the core with its last key counted twice, 0 with its last key dropped."""
    q, k, v, do = q.double(), k.double(), v.double(), do_heads.double()
    w = torch.ones(k.shape[1], dtype=torch.float64, device=k.device)
    w[-1] = last_key_weight
    s = torch.bmm(q, k.transpose(1, 2))
    m = s.amax(dim=-1, keepdim=True)
    e = torch.exp(s - m) * w
    l = e.sum(dim=-1, keepdim=True)
    p = e / l
    out = torch.bmm(p, v)
    lse = (m + torch.log(l)).squeeze(-1)
    dp = torch.bmm(do, v.transpose(1, 2))
    delta = (do * out).sum(dim=-1, keepdim=True)
    ds = p * (dp - delta)
    return out, lse, torch.bmm(ds, k), torch.bmm(ds.transpose(1, 2), q), torch.bmm(p.transpose(1, 2), do)


def _bf(x):
    return x.to(torch.bfloat16).double()


def attn_emul_bf16(q, k, v, do_heads):
    """The kernels' rounding points in float64 arithmetic (module docstring); same returns as attn_ref64."""
    q, k, v, do = q.double(), k.double(), v.double(), do_heads.double()
    s = torch.bmm(q, k.transpose(1, 2))
    m = s.amax(dim=-1, keepdim=True)
    pb = _bf(torch.exp(s - m))                      # P rounded to bf16 before the row sum and before P.V
    l = pb.sum(dim=-1, keepdim=True)
    out = _bf(torch.bmm(pb, v) / l)                 # stored in bf16
    lse = (m + torch.log(l)).float().double()       # stored in f32
    delta = (do * out).sum(dim=-1, keepdim=True)    # from the STORED out
    p = torch.exp(s - lse)
    dp = torch.bmm(do, v.transpose(1, 2))
    dsb, pb2 = _bf(p * (dp - delta)), _bf(p)        # dS and P rounded to bf16 before the gradient products
    return (out, lse.squeeze(-1), _bf(torch.bmm(dsb, k)), _bf(torch.bmm(dsb.transpose(1, 2), q)),
            _bf(torch.bmm(pb2.transpose(1, 2), do)))


def deviations(got, ref):
    """the five figures the gates apply to: out max-rel, lse max-abs, rel-L2 of dq, dk, dv"""
    return (max_rel(got[0], ref[0]), float((got[1] - ref[1]).abs().max()), rel_err(got[2], ref[2]), rel_err(got[3], ref[3]),
            rel_err(got[4], ref[4]))


GATES = (OUT_GATE, LSE_GATE, GRAD_GATE, GRAD_GATE, GRAD_GATE)
NAMES = ("out", "lse", "dq", "dk", "dv")


@pytest.mark.parametrize("N", SWEEP_N)
def test_sweep_gates_sit_between_the_rounding_floor_and_an_off_by_one_key_mask(N):
    Bt, H = SWEEP_BT, SWEEP_H
    q, k, v, do = sweep_inputs(N)
    doh = heads_of(do, Bt, H, N)
    ref = attn_ref64(q, k, v, doh)
    floor = deviations(attn_emul_bf16(q, k, v, doh), ref)
    twice = deviations(attn_ref64(q, k, v, doh, 2.0), ref)
    dropped = deviations(attn_ref64(q, k, v, doh, 0.0), ref)
    print(f"\nN={N:3d} floor   " + "  ".join(f"{n} {x:.2e}" for n, x in zip(NAMES, floor)))
    print(f"N={N:3d} twice   " + "  ".join(f"{n} {x:.2e}" for n, x in zip(NAMES, twice)))
    print(f"N={N:3d} dropped " + "  ".join(f"{n} {x:.2e}" for n, x in zip(NAMES, dropped)))
    for n, f, t, d, gate in zip(NAMES, floor, twice, dropped, GATES):
        assert f < gate, f"{n}: the bf16 rounding floor {f:.3e} is not below the gate {gate}"
        assert t > gate, f"{n}: the last key counted twice moves it by {t:.3e} only (gate {gate})"
        assert d > gate, f"{n}: the last key dropped moves it by {d:.3e} only (gate {gate})"


def test_layout_helpers_are_inverse():
    Bt, H, N = 2, 3, 5
    rows = torch.arange(Bt * N * H * 64, dtype=torch.float32).reshape(Bt * N, H * 64)
    assert torch.equal(rows_of(heads_of(rows, Bt, H, N), Bt, H, N), rows)
    assert heads_of(rows, Bt, H, N)[1 * H + 2, 3, 7] == rows[1 * N + 3, 2 * 64 + 7]
