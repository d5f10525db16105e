"""Host side of tests/test_gpu_lowrank.py (no GPU): the inputs of the per-launch tests of the attention-site low-rank adapter kernels
(csrc/lowrank.hip: prep_kadapt, prep_lora, lowrank_u, lowrank_grad, lowrank_combo, lowrank_reduce, chain_kadapt, rule_sum, chain_lora,
and the f32 twins of csrc/verify.hip), their float64 references, the assertions themselves, the rounding floors the GPU gates are
taken from, and the evidence that the assertions can see what they are meant to see.  The kernels are nowhere in sight here: the
emulation is the reference, never the kernel.

Layouts (lowrank.hip states them).  Internal rows are batch-major, row = b*N + n; the reference's raw reshape makes reference row
rr = n*B + b of the delta the flat elements [rr*E, rr*E + E) of the head-layout (B, H, N, 64) q / v buffer.  `case` draws dDelta in
that flat view and maps it to the row layout of dqkv ([T][3E + 64]: dq | dk | dv | the bf16 copy of u).

  * input recipe (`case`, seeded by the shape, never modified): bf16 dDelta_q / dDelta_v, xn, a bf16 Q panel, f32 t; the last
    reference row (== the last internal row) of dDelta, xn and t is doubled, and so is that row of u = dDelta Q: a tail row that is
    dropped or counted twice moves whole columns of a per-chunk partial.  `chain_case`: non-zero bias partials and non-zero
    gradients already in the buffer (the chain kernels accumulate with +=), phm_rule factors in +-1.
  * float64 references: u (`u64`), the per-256-row-chunk partials dP = xn^T bf16(u), dQ = dDelta^T bf16(t) and the d bias column
    sums (`grad64`; the totals are their sums), the reduce (`reduce64`, `bias64`), the chain rules (`chain_kadapt64`, and the LoRA
    rule inside `chain_expected`), `rule_sum64`, and the preps twice: as the kernels state them (rank-1 factors, `prep_factors` /
    `prep_panels` in float64) and from the reference model's
    H = sum_i kron(rule_i, W_i), shown equal to P Q^T (test_kron_definition_equals_the_rank32_panels); the KAdaptation chain rule is
    checked against torch.autograd through that kron construction (test_chain_rule_equals_autograd_through_the_kron_definition).
  * emulations with the kernels' rounding points.  u and the partials: bf16 operands (their products are exact in f32) summed in
    f32 ONE PRODUCT AT A TIME -- K roundings per element, an upper model of any f32 accumulator that rounds to nearest (the matrix
    core rounds once per 8..32 products) -- `seq=True`.  reduce and rule_sum: the documented trees in torch float32 (`reduce32`,
    `rule_sum32`): element-wise IEEE additions in a fixed order, so the kernels' outputs must have THEIR BITS.  chain rules: torch
    float32 in the kernels' loop order without fused multiply-add (`chain_kadapt32`).  preps: the kernels' operation order in torch
    float32, ascale * (rule * l), then one round-to-nearest-even to bf16 (`prep_panels` in float32): bit-identical again.
  * floors = emulation against float64, per shape, max-rel (per chunk and plane where the output has chunks).  Measured here
    (`pytest -s` prints them):
        u32            6.9e-8 (T = 1) .. 4.4e-7 (T = 394, E = 768)              partial planes   0 (T = 1: one exact product) .. 3.5e-7
        d bias partial 0 (T <= 60: exact sums) .. 4.7e-8                         f32 twins        u as above, partial 4.5e-8 .. 6.3e-7
        reduce G       0 (one chunk) .. 1.2e-7, bias 6.2e-8 .. 2.7e-7             chain KAdaptation 1.7e-7 .. 3.1e-7, LoRA 6.3e-8 .. 1.1e-7
        rule_sum       3.5e-8 .. 1.5e-7                                          preps bf16 2.0e-3 .. 3.7e-3 (half a bf16 ulp: 2^-8), f32 <= 9.4e-8
    GPU gate = FLOOR_FACTOR x max(floor, 2^-24), FLOOR_FACTOR = 2, the house factor: nothing here rounds a tie differently in f32 and
    f64 (bf16(u) and bf16(t) are taken from the f32 values the kernel is given, not from float64), so the CPU run shows no tie-flip
    noise and no larger factor is needed.  2^-24 is half an f32 ulp of the largest element: the output format itself, below which no
    f32 store can promise anything (it matters where the emulation is exact: T = 1, a one-row chunk).  Every gate is capped by the
    existing ones: 2e-4 for u32 and the partials (test_lowrank_u_and_grads), 2e-5 for pure-f32 outputs, 1e-2 for bf16 panels.
  * the bite (test_the_assertions_bite_u_and_partials, test_reduce_and_chain_floors_and_bite, test_rule_sum_floor_and_bite,
    test_prep_floors_and_bite): each wrong kernel below, as a mutant of the emulation, must FAIL the assertions at every
    shape of the grid at which it differs from the right kernel at all; the unmutated emulation must pass.
      (a) row map without the n/b swap (identity at B = 1)        (b) the last valid row of the last chunk dropped
      (c) all pad rows of the last chunk counted as copies of row T - 1 (no pad rows at T % 256 == 0)
      (d) the q and v planes of `partial` swapped                  (e) d bias from one of the two planes only
      (f) the reduce skipping chunk 8, the first chunk of the second round (chunks >= 9)
      (g) rule_sum missing layer l_lo; rule_sum overwriting instead of starting from the value already there
      (h) LoRA pad columns j >= r not zeroed in the panels (r < 32) (i) ascale applied to dP but not to dQ
      (j) bf16 truncation instead of round-to-nearest in the prep stores
"""
import functools

import pytest
import torch

from conftest import max_rel
from test_adapter_fused_host import bf16_trunc

LG_ROWS = 256                               # token rows per chunk of the gradient kernels (== pevit_op_lowrank_chunks' divisor)
GRID = [(1, 1, 1), (3, 5, 1), (6, 10, 2), (1, 257, 2), (2, 128, 5), (1, 50, 12), (2, 197, 12), (1, 257, 16)]      # (B, N, H), E = 64 H
F32_SHAPES = GRID[:5]                       # the f32 twins: the small shapes
PREP_E = (64, 128, 768, 1024)
LORA_R = (1, 4, 8, 32)
REDUCE_CHUNKS = (1, 7, 8, 9, 16, 17, 25)
CHAIN_LORA_R = (1, 8, 32)
RULE_RANGES = ((0, 1), (0, 8), (0, 9), (3, 12), (0, 24))
LAYERS = 3
ASCALE = 160.0
FLOOR_FACTOR = 2.0
ULP = 2.0 ** -24                            # half an f32 ulp of the largest element
MFMA_GATE, F32_GATE, BF16_GATE = 2e-4, 2e-5, 1e-2       # the existing gates: caps of the floor gates
BF = torch.bfloat16
F64 = torch.float64


def gate_of(floor, cap):
    return min(cap, FLOOR_FACTOR * max(floor, ULP))


# ---------------------------------------------------------------------------------------------------------------- layouts
def ref_rows(B, N, device="cpu"):
    """idx[rr] = internal row b*N + n of reference row rr = n*B + b"""
    rr = torch.arange(B * N, device=device)
    return (rr % B) * N + rr // B


def rows_of_flat(flat, B, N, H):
    """the reference's (rr, e) view of a head-layout buffer -> the row layout [b*N + n][h*64 + d]"""
    return flat.view(B, H, N, 64).permute(0, 2, 1, 3).reshape(B * N, H * 64)


def flat_of_rows(rows, B, N, H):
    return rows.reshape(B, N, H, 64).permute(0, 2, 1, 3).reshape(B * N, H * 64)


def chunks_of(T):
    return -(-T // LG_ROWS)


# ---------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def case(B, N, H):
    g = torch.Generator(device="cpu").manual_seed(100000 * B + 100 * N + H)

    def R(*s, sc=1.0):
        return torch.randn(*s, generator=g) * sc
    T, E = B * N, 64 * H
    c = dict(B=B, N=N, H=H, T=T, E=E)
    for k in ("ddq", "ddv"):                 # flat view, rows rr
        x = R(T, E)
        x[-1] *= 2
        c[k] = x.to(BF)
    c["dk_rows"] = R(T, E).to(BF)
    c["q32"] = R(E, 64, sc=0.3).to(BF).float()      # the f32 panel holds the bf16 values: both u kernels see the same Q
    c["qT"] = c["q32"].t().contiguous().to(BF)
    xn = R(T, E)
    xn[-1] *= 2
    c["xn"] = xn.to(BF)
    t = R(T, 64)
    t[-1] *= 2
    c["t"] = t
    c["dq_rows"] = rows_of_flat(c["ddq"], B, N, H).contiguous()
    c["dv_rows"] = rows_of_flat(c["ddv"], B, N, H).contiguous()
    c["u32"] = u64(c).float()               # the operand of the gradient kernels: from float64, not from the u kernel
    return c


def on(c, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in c.items()}


# ---------------------------------------------------------------------------------------------------------------- u
def seq_matmul(A, Bm):
    """A [M][K] @ Bm [K][J] in f32, one product at a time in k order (K roundings per element)"""
    acc = torch.zeros((A.shape[0], Bm.shape[1]), dtype=torch.float32, device=A.device)
    A, Bm = A.float(), Bm.float()
    for k in range(A.shape[1]):
        acc = acc + A[:, k:k + 1] * Bm[k:k + 1, :]
    return acc


def u64(c, seq=False, swap=True):
    """u [T][64] in internal row order; seq: the f32 emulation; swap=False: mutant (a)"""
    Q = c["q32"]
    mm = seq_matmul if seq else (lambda a, b: a.double() @ b.double())
    uf = torch.cat([mm(c["ddq"], Q[:, :32]), mm(c["ddv"], Q[:, 32:])], dim=1)
    if not swap:
        return uf
    out = torch.empty_like(uf)
    out[ref_rows(c["B"], c["N"], uf.device)] = uf
    return out


def check_u(c, u32, ucols, gate):
    """u32 [T][64] f32 against float64; ucols [T][64] bf16 must be bf16(u32) bit for bit (one f32 value feeds both stores)"""
    assert torch.isfinite(u32).all(), "u32: an element was left unwritten"
    fig = max_rel(u32, u64(c))
    assert fig <= gate, f"u32: {fig:.3e} > {gate:.3e}"
    if ucols is not None:
        assert ucols.dtype == BF and torch.equal(ucols.contiguous().view(torch.int16), u32.to(BF).view(torch.int16)), \
            "the bf16 copy of u is not bf16(u32)"
    return fig


# ---------------------------------------------------------------------------------------------------------------- partials
def chunked(x, T):
    """[T][W] -> [chunks][256][W], zero rows behind T"""
    ch = chunks_of(T)
    pad = torch.zeros((ch * LG_ROWS, x.shape[1]), dtype=x.dtype, device=x.device)
    pad[:T] = x
    return pad.view(ch, LG_ROWS, -1)


def contract(X, Y, seq):
    """[ch][256][E], [ch][256][J] -> [ch][E][J]: sum over the rows of each chunk"""
    if not seq:
        return torch.einsum("cre,crj->cej", X.double(), Y.double())
    X, Y = X.float(), Y.float()
    acc = torch.zeros((X.shape[0], X.shape[2], Y.shape[2]), dtype=torch.float32, device=X.device)
    for r in range(X.shape[1]):
        acc = acc + X[:, r, :, None] * Y[:, r, None, :]
    return acc


def colsum(X, seq):
    if not seq:
        return X.double().sum(1)
    X = X.float()
    acc = torch.zeros((X.shape[0], X.shape[2]), dtype=torch.float32, device=X.device)
    for r in range(X.shape[1]):
        acc = acc + X[:, r]
    return acc


def grad64(c, u32=None, seq=False, swap=True, row_weight=None, swap_planes=False, f32_operands=False):
    """partial [chunks][4][E][32] (dP_q, dP_v, dQ_q, dQ_v) and dbias_partial [chunks][2][E] from the given u32 (default: the case's).
    The matrix-core kernels round u and t to bf16 (f32_operands: the f32 twins do not).  swap=False: mutant (a); row_weight [T]: how
    often a row is counted, mutants (b), (c); swap_planes: mutant (d)"""
    B, N, T = c["B"], c["N"], c["T"]
    u32 = c["u32"] if u32 is None else u32
    dev = u32.device
    rnd = (lambda x: x) if f32_operands else (lambda x: x.to(BF).float())
    w = torch.ones(T, device=dev) if row_weight is None else row_weight.to(dev).float()
    t_ref = c["t"][ref_rows(B, N, dev)] if swap else c["t"]
    xw, qw, vw = (chunked(x.float() * w[:, None], T) for x in (c["xn"], c["ddq"], c["ddv"]))
    uy, ty = chunked(rnd(u32), T), chunked(rnd(t_ref), T)
    planes = [contract(xw, uy[..., :32], seq), contract(xw, uy[..., 32:], seq), contract(qw, ty[..., :32], seq), contract(vw, ty[..., 32:], seq)]
    if swap_planes:
        planes = [planes[1], planes[0], planes[3], planes[2]]
    return torch.stack(planes, dim=1), torch.stack([colsum(qw, seq), colsum(vw, seq)], dim=1)


def planewise(got, ref, lead=2):
    """max over the `lead` leading dimensions (chunk, plane) of max|got - ref| / max|ref| taken over the pair's own elements"""
    g, r = got.double(), ref.double()
    d = (g - r).abs().flatten(lead).amax(-1)
    return float((d / (r.abs().flatten(lead).amax(-1) + 1e-30)).max())


def grad_figures(partial, dbias, ref):
    rp, rb = ref
    assert partial.shape == rp.shape and dbias.shape == rb.shape, (partial.shape, rp.shape, dbias.shape, rb.shape)
    return dict(partial=planewise(partial, rp), dbias=planewise(dbias, rb),
                total=planewise(partial.double().sum(0), rp.sum(0), lead=1), dbias_total=max_rel(dbias.double().sum((0, 1)), rb.sum((0, 1))))


def check_grad(c, partial, dbias, gates, u32=None, f32_operands=False, dp_only=False):
    """every chunk's planes and bias sums, and their totals, against float64; gates: dict like grad_figures'.  dp_only: the
    launch wrote the dP planes alone (the deferred product of lowrank_combo)"""
    ref = grad64(c, u32, f32_operands=f32_operands)
    if dp_only:
        partial, dbias, ref = partial[:, :2], ref[1], (ref[0][:, :2], ref[1])
    assert torch.isfinite(partial).all() and torch.isfinite(dbias).all(), "an element was left unwritten"
    fig = grad_figures(partial, dbias, ref)
    for k, v in fig.items():
        assert v <= gates[k], f"{k}: {v:.3e} > {gates[k]:.3e}"
    return fig


@functools.lru_cache(maxsize=None)
def floors_cpu(B, N, H):
    return floors(case(B, N, H))


def floors(c, f32_operands=False):
    """{u, partial, dbias, total, dbias_total}: the f32 one-product-at-a-time emulation against float64"""
    fl = dict(u=max_rel(u64(c, seq=True), u64(c)))
    p, b = grad64(c, seq=True, f32_operands=f32_operands)
    fl.update(grad_figures(p, b, grad64(c, f32_operands=f32_operands)))
    return fl


def gates(fl, cap=MFMA_GATE):
    return {k: gate_of(v, cap) for k, v in fl.items()}


# ---------------------------------------------------------------------------------------------------------------- reduce
def reduce32(partial, skip=None):
    """the tree of lowrank_reduce_kernel in torch float32: eight running sums over the chunks c = u (mod 8) in rising order,
    then ((0+1)+(2+3))+((4+5)+(6+7)).  partial [chunks][n]; skip: mutant (f)"""
    z = torch.zeros_like(partial[0])
    s = [z.clone() for _ in range(8)]
    for ch in range(partial.shape[0]):
        if ch != skip:
            s[ch % 8] = s[ch % 8] + partial[ch]
    return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]))


def bias32(dbias, start, one_plane=False):
    """g_b += sum over the chunks in order of (plane 0 + plane 1).  dbias [chunks][2][E]; one_plane: mutant (e)"""
    s = torch.zeros_like(start)
    for ch in range(dbias.shape[0]):
        s = s + (dbias[ch, 0] if one_plane else dbias[ch, 0] + dbias[ch, 1])
    return start + s


def reduce64(partial):
    return partial.double().sum(0)


def bias64(dbias, start):
    return start.double() + dbias.double().sum((0, 1))


def check_reduce(G, partial, gb, dbias, gb_start, gate_G, gate_b, cols=32):
    """G [4*E*32] of one layer: the bits of the documented tree, and float64 within the gate; gb likewise (None: no bias).
    cols < 32 (LoRA): only the columns j < cols of G and of the partials are looked at"""
    if cols < 32:
        G, partial = (x.reshape(x.shape[:-1] + (-1, 32))[..., :cols].reshape(x.shape[:-1] + (-1,)) for x in (G, partial))
    assert torch.isfinite(G).all(), "G: an element was left unwritten"
    assert torch.equal(G.contiguous().view(torch.int32), reduce32(partial).contiguous().view(torch.int32)), "G does not have the bits of the documented tree"
    fig = dict(G=max_rel(G, reduce64(partial)))
    assert fig["G"] <= gate_G, fig
    if gb is not None:
        assert torch.equal(gb.view(torch.int32), bias32(dbias, gb_start).view(torch.int32)), "d bias does not have the bits of the chunk-order sum"
        fig["bias"] = max_rel(gb, bias64(dbias, gb_start))
        assert fig["bias"] <= gate_b, fig
    return fig


# ---------------------------------------------------------------------------------------------------------------- chain rules
@functools.lru_cache(maxsize=None)
def chain_case(E, chunks, method, r=32, L=LAYERS):
    """partials of L layers with strides larger than compact, the flat parameter and gradient buffers"""
    g = torch.Generator(device="cpu").manual_seed(7 * E + 131 * chunks + 1000 * r + (0 if method == "kadaptation" else 1))

    def R(*s, sc=1.0):
        return torch.randn(*s, generator=g) * sc
    plane = 4 * E * 32
    c = dict(E=E, chunks=chunks, method=method, r=r, L=L, partial_layer=(chunks + 1) * plane + 64, dbias_layer=chunks * 2 * E + 32)
    part = torch.full((L, c["partial_layer"]), float("nan"))
    pay = R(L, chunks, 4, E, 32)
    if method == "lora":
        pay[..., r:] = float("nan")         # the pad columns of the panels: whatever the contraction left there must not leak
    part[:, :chunks * plane] = pay.view(L, -1)
    c["partial"] = part
    db = torch.full((L, c["dbias_layer"]), float("nan"))
    db[:, :chunks * 2 * E] = R(L, chunks * 2 * E, sc=3.0) + 0.5
    c["dbias"] = db
    per_layer = 5 * E if method == "kadaptation" else 4 * r * E
    c["p_layer0"], c["p_layer_stride"] = 4096 + 64, per_layer + 24
    n = c["p_layer0"] + L * c["p_layer_stride"] + 16
    params = R(n, sc=0.5)
    params[:4096] = torch.where(R(4096) < 0, -1.0, 1.0)          # phm_rule factors in +-1
    c["params"] = params
    c["grads0"] = R(n, sc=0.7) + 0.1                              # what is already in the gradient buffer
    return c


def layer_partial(c, l):
    E, ch = c["E"], c["chunks"]
    return c["partial"][l, :ch * 4 * E * 32].view(ch, 4 * E * 32), c["dbias"][l, :ch * 2 * E].view(ch, 2, E)


def chain_kadapt64(G, rule, ql, qr, ascale=ASCALE, dq_scale=None, dtype=F64):
    """G [4][E][32]; rule [4][32][32] = s1, t1, s2, t2 (rows j); ql, qr [32][F].  Returns d rule [4][32][32] (what one layer puts into
    rule_scratch) and the increments of q_left, q_right [32][F].  dq_scale: mutant (i), the factor on the dQ side"""
    E = G.shape[1]
    F = E // 32
    Gv = G.to(dtype).view(4, 32, F, 32)     # [plane][a][k][j]
    s1, t1, s2, t2 = (x.to(dtype) for x in rule)
    ql, qr = ql.to(dtype), qr.to(dtype)
    aq = ascale if dq_scale is None else dq_scale
    d = torch.stack([ascale * torch.einsum("akj,jk->ja", Gv[0], ql), aq * torch.einsum("cpj,jp->jc", Gv[2], qr),
                     ascale * torch.einsum("akj,jk->ja", Gv[1], ql), aq * torch.einsum("cpj,jp->jc", Gv[3], qr)])
    dl = ascale * (torch.einsum("akj,ja->jk", Gv[0], s1) + torch.einsum("akj,ja->jk", Gv[1], s2))
    dr = aq * (torch.einsum("cpj,jc->jp", Gv[2], t1) + torch.einsum("cpj,jc->jp", Gv[3], t2))
    return d, dl, dr


def chain_kadapt32(G, rule, ql, qr, ascale=ASCALE):
    """the loops of chain_kadapt_kernel in torch float32, a product and an addition at a time (no fused multiply-add)"""
    E = G.shape[1]
    F = E // 32
    Gv = G.float().view(4, 32, F, 32)
    s1, t1, s2, t2 = (x.float() for x in rule)
    z = lambda *s: torch.zeros(*s)
    d = [z(32, 32) for _ in range(4)]
    for k in range(F):                       # [j][a] += G[a][k][j] * l[j][k]
        d[0] = d[0] + Gv[0][:, k, :].t() * ql[:, k:k + 1]
        d[2] = d[2] + Gv[1][:, k, :].t() * ql[:, k:k + 1]
        d[1] = d[1] + Gv[2][:, k, :].t() * qr[:, k:k + 1]
        d[3] = d[3] + Gv[3][:, k, :].t() * qr[:, k:k + 1]
    dl, dr = z(32, F), z(32, F)
    for a in range(32):                      # [j][k] += G0[a][k][j] * s1[j][a] + G1[a][k][j] * s2[j][a]
        dl = dl + (Gv[0][a].t() * s1[:, a:a + 1] + Gv[1][a].t() * s2[:, a:a + 1])
        dr = dr + (Gv[2][a].t() * t1[:, a:a + 1] + Gv[3][a].t() * t2[:, a:a + 1])
    return torch.stack([ascale * x for x in d]), ascale * dl, ascale * dr


def kadapt_layer_params(c, l, buf=None):
    E = c["E"]
    o = c["p_layer0"] + l * c["p_layer_stride"]
    buf = c["params"] if buf is None else buf
    return buf[o:o + E].view(32, E // 32), buf[o + E:o + 2 * E].view(32, E // 32)


def chain_expected(c, G, dtype=F64, chain=None, **mutant):
    """the gradient buffer and rule_scratch [L][4096] after the chain launch, from G [L][4][E][32] (the reduce's output) and the
    bias sums of the case: (grads, scratch, mask of the gradient elements the launch writes)"""
    E, L, r = c["E"], c["L"], c["r"]
    grads = c["grads0"].to(dtype).clone()
    mask = torch.zeros(grads.shape, dtype=torch.bool)
    scratch = torch.zeros((L, 4096), dtype=dtype)
    for l in range(L):
        o = c["p_layer0"] + l * c["p_layer_stride"]
        if c["method"] == "kadaptation":
            ql, qr = kadapt_layer_params(c, l)
            d, dl, dr = (chain or chain_kadapt64)(G[l], c["params"][:4096].view(4, 32, 32), ql, qr, **mutant)
            scratch[l] = d.reshape(-1).to(dtype)
            grads[o:o + E] += dl.reshape(-1).to(dtype)
            grads[o + E:o + 2 * E] += dr.reshape(-1).to(dtype)
            _, db = layer_partial(c, l)
            grads[o + 4 * E:o + 5 * E] = (bias64 if dtype == F64 else bias32)(db, c["grads0"][o + 4 * E:o + 5 * E])
            mask[o:o + 2 * E] = True
            mask[o + 4 * E:o + 5 * E] = True
        else:
            Gl = G[l].to(dtype)[:, :, :r]
            aq = mutant.get("dq_scale", ASCALE)
            rE = r * E
            grads[o:o + rE] += ASCALE * Gl[0].t().reshape(-1)                     # a1q [r][E]
            grads[o + rE:o + 2 * rE] += aq * Gl[2].reshape(-1)                    # a2q [E][r]
            grads[o + 2 * rE:o + 3 * rE] += ASCALE * Gl[1].t().reshape(-1)
            grads[o + 3 * rE:o + 4 * rE] += aq * Gl[3].reshape(-1)
            mask[o:o + 4 * rE] = True
    return grads, scratch, mask


def check_chain(c, grads, scratch, G, gate):
    """grads (whole buffer), scratch [L][4096] (KAdaptation) after the launch, against the float64 chain of the reduce's own G"""
    exp, exp_s, mask = chain_expected(c, G.cpu() if G.is_cuda else G)
    grads = grads.cpu()
    assert torch.equal(grads[~mask].view(torch.int32), c["grads0"][~mask].view(torch.int32)), "an element outside the layers' tensors was written"
    assert torch.isfinite(grads).all(), "a NaN of the pad columns or of the stride padding leaked into the gradients"
    fig = {}
    L, E, r = c["L"], c["E"], c["r"]
    for l in range(L):
        o = c["p_layer0"] + l * c["p_layer_stride"]
        spans = (dict(q_left=(o, o + E), q_right=(o + E, o + 2 * E), bias=(o + 4 * E, o + 5 * E)) if c["method"] == "kadaptation" else
                 {n: (o + i * r * E, o + (i + 1) * r * E) for i, n in enumerate(("a1q", "a2q", "a1v", "a2v"))})
        for n, (a, b) in spans.items():
            fig[n] = max(fig.get(n, 0.0), max_rel(grads[a:b], exp[a:b]))
    if c["method"] == "kadaptation":
        s = scratch.cpu()
        assert torch.isfinite(s).all()
        for i, n in enumerate(("rule1_l", "rule1_r", "rule2_l", "rule2_r")):
            fig[n] = max(max_rel(s[l].view(4, 1024)[i], exp_s[l].view(4, 1024)[i]) for l in range(L))
    for k, v in fig.items():
        assert v <= gate, f"{k}: {v:.3e} > {gate:.3e}"
    return fig


def reduced(c):
    """G [L][4][E][32] in f32: the documented tree applied to the case's partials"""
    return torch.stack([reduce32(layer_partial(c, l)[0]).view(4, c["E"], 32) for l in range(c["L"])])


def chain_floor(c):
    """the float32 chain against the float64 chain, both from the same f32 G: largest max-rel over the tensors"""
    G = torch.nan_to_num(reduced(c))
    got, got_s, _ = chain_expected(c, G, dtype=torch.float32, chain=chain_kadapt32 if c["method"] == "kadaptation" else None)
    return check_chain(c, got, got_s, G, gate=1.0)


@functools.lru_cache(maxsize=None)
def chain_gates(E, chunks, method, r=32):
    """(gate of G, gate of the bias gradient, gate of the chain outputs) of a chain_case: its float32 floors x FLOOR_FACTOR"""
    c = chain_case(E, chunks, method, r)
    fG = fb = 0.0
    for l in range(c["L"]):
        part, db = layer_partial(c, l)
        part = torch.nan_to_num(part)
        fG = max(fG, max_rel(reduce32(part), reduce64(part)))
        if method == "kadaptation":
            o = c["p_layer0"] + l * c["p_layer_stride"] + 4 * E
            fb = max(fb, max_rel(bias32(db, c["grads0"][o:o + E]), bias64(db, c["grads0"][o:o + E])))
    return gate_of(fG, F32_GATE), gate_of(fb, F32_GATE), gate_of(max(chain_floor(c).values()), F32_GATE)


# ---------------------------------------------------------------------------------------------------------------- rule_sum
@functools.lru_cache(maxsize=None)
def rule_case(layers=24):
    g = torch.Generator(device="cpu").manual_seed(4096)
    return dict(scratch=torch.randn(layers, 4096, generator=g), start=torch.randn(4096, generator=g) + 0.25)


def rule_sum32(scratch, start, l_lo, l_hi, miss_lo=False, overwrite=False):
    """one running sum from the value already there, top layer first; mutants (g)"""
    s = torch.zeros_like(start) if overwrite else start.clone()
    for l in range(l_hi - 1, l_lo - 1 + (1 if miss_lo else 0), -1):
        s = s + scratch[l]
    return s


def rule_sum64(scratch, start, l_lo, l_hi):
    return start.double() + scratch[l_lo:l_hi].double().sum(0)


def check_rule_sum(got, scratch, start, l_lo, l_hi, gate):
    assert torch.isfinite(got).all(), "a layer outside [l_lo, l_hi) was read"
    fig = max_rel(got, rule_sum64(scratch, start, l_lo, l_hi))
    assert fig <= gate, f"rule_sum: {fig:.3e} > {gate:.3e}"
    return fig


# ---------------------------------------------------------------------------------------------------------------- preps
PANELS = ("w_aug_rows", "wT_aug_cols", "q32", "qT", "q16")


@functools.lru_cache(maxsize=None)
def prep_case(E, method, r=32, L=LAYERS):
    g = torch.Generator(device="cpu").manual_seed(3 * E + r + (0 if method == "kadaptation" else 50000))

    def R(*s, sc=1.0):
        return torch.randn(*s, generator=g) * sc
    per_layer = 2 * E if method == "kadaptation" else 4 * r * E
    c = dict(E=E, method=method, r=r, L=L, param_floats=per_layer + 40)
    c["rule"] = torch.where(R(4, 32, 32) < 0, -1.0, 1.0) * (1 + 0.25 * torch.rand(4, 32, 32, generator=g))    # s1, t1, s2, t2
    c["layer_params"] = R(L, c["param_floats"], sc=0.05)
    return c


def prep_factors(c, l, dtype):
    """P_q, P_v, Q_q, Q_v [E][32] of layer l as the kernels state them, in `dtype` arithmetic"""
    E, r = c["E"], c["r"]
    p = c["layer_params"][l].to(dtype)
    if c["method"] == "kadaptation":
        F = E // 32
        ql, qr = p[:E].view(32, F), p[E:2 * E].view(32, F)
        s1, t1, s2, t2 = (x.to(dtype) for x in c["rule"])
        kr = lambda s, w: (s[:, :, None] * w[:, None, :]).reshape(32, E).t()        # [e = a*F + k][j] = s[j][a] * w[j][k]
        return kr(s1, ql), kr(s2, ql), kr(t1, qr), kr(t2, qr)
    rE = r * E
    pad = lambda x: torch.cat([x, torch.zeros((E, 32 - r), dtype=dtype)], dim=1)
    return (pad(p[:rE].view(r, E).t()), pad(p[2 * rE:3 * rE].view(r, E).t()), pad(p[rE:2 * rE].view(E, r)), pad(p[3 * rE:4 * rE].view(E, r)))


def prep_panels(c, l, dtype=torch.float32, f32=False, q=None, dirty_pad=False, ascale=ASCALE):
    """the five panels of layer l: dtype float32 = the kernels' operation order, ascale * (rule * l), stored with q (default:
    round to nearest even to bf16; f32 storage stores as is); float64 = the reference.  dirty_pad: mutant (h)"""
    Pq, Pv, Qq, Qv = prep_factors(c, l, dtype)
    if dirty_pad and c["method"] == "lora" and c["r"] < 32:
        for x in (Pq, Pv, Qq, Qv):
            x[:, c["r"]:] = x[:, :1]
    Pm, Qm = torch.cat([Pq, Pv], 1), torch.cat([Qq, Qv], 1)         # [E][64]
    if dtype == F64:
        store = lambda x: x
    elif f32:
        store = lambda x: x
    else:
        store = q or (lambda x: x.to(BF))
    out = dict(w_aug_rows=store(Pm.t().contiguous()), wT_aug_cols=store(ascale * Pm), q32=Qm.clone(), qT=store(Qm.t().contiguous()))
    if not f32 or dtype == F64:
        out["q16"] = store(Qm)
    return out


def trunc_store(x):
    return bf16_trunc(x.double()).to(BF)


def check_prep(c, l, got, f32, gate):
    """got: the panels of layer l as the launch left them ([64][E], [E][64], ...).  Each has the bits of the float32 evaluation in
    the kernels' operation order and lies within the gate of float64; q16 == bf16(q32), qT == q16^T; LoRA: pad columns are +0"""
    emu, ref = prep_panels(c, l, f32=f32), prep_panels(c, l, dtype=F64)
    fig = {}
    for k, e in emu.items():
        g = got[k]
        assert g.dtype == e.dtype and g.shape == e.shape, (k, g.dtype, g.shape)
        it = torch.int16 if g.dtype == BF else torch.int32
        assert torch.equal(g.contiguous().view(it), e.contiguous().view(it)), f"{k}: not the bits of the float32 evaluation"
        fig[k] = max_rel(g, ref[k])
        assert fig[k] <= gate[k], f"{k}: {fig[k]:.3e} > {gate[k]:.3e}"
    if not f32:
        assert torch.equal(got["q16"].view(torch.int16), got["q32"].to(BF).view(torch.int16)), "q16 != bf16(q32)"
        assert torch.equal(got["qT"].view(torch.int16), got["q16"].t().contiguous().view(torch.int16)), "qT != q16^T"
    if c["method"] == "lora":
        r = c["r"]
        for k in emu:
            g = got[k]
            pads = torch.cat([g[r:32], g[32 + r:]]) if k in ("w_aug_rows", "qT") else torch.cat([g[:, r:32], g[:, 32 + r:]], 1)
            it = torch.int16 if g.dtype == BF else torch.int32
            assert not bool(pads.contiguous().view(it).any()), f"{k}: a pad column j >= r is not +0"
    return fig


def prep_floor(c, f32):
    fl = {}
    for l in range(c["L"]):
        emu, ref = prep_panels(c, l, f32=f32), prep_panels(c, l, dtype=F64)
        for k in emu:
            fl[k] = max(fl.get(k, 0.0), max_rel(emu[k], ref[k]))
    return fl


def prep_gates(c, f32):
    return {k: gate_of(v, F32_GATE if (f32 or k == "q32") else BF16_GATE) for k, v in prep_floor(c, f32).items()}


# ---------------------------------------------------------------------------------------------------------------- tests
def _fails(fn, *a, **k):
    try:
        fn(*a, **k)
    except AssertionError:
        return True
    return False


def test_row_maps_are_inverse_and_match_the_raw_reshape():
    B, N, H = 3, 5, 2
    idx = ref_rows(B, N)
    assert sorted(idx.tolist()) == list(range(B * N)) and idx[1] == N and idx[B] == 1
    x = torch.arange(B * N * H * 64, dtype=torch.float32).view(B * N, H * 64)
    assert torch.equal(flat_of_rows(rows_of_flat(x, B, N, H), B, N, H), x)
    rows = rows_of_flat(x, B, N, H)          # flat element i lives at head-layout (bh = i // 64 // N, n = i // 64 % N, d = i % 64)
    i = 64 * (N + 2) + 7
    assert rows[0 * N + 2, 1 * 64 + 7] == i


@pytest.mark.parametrize("B,N,H", GRID)
def test_floors_and_the_emulation_passes(B, N, H):
    """the one-product-at-a-time f32 emulation against float64 (the floors of the GPU gates), and the emulation held to the
    assertions of the GPU file at those gates"""
    c = case(B, N, H)
    fl = floors_cpu(B, N, H)
    print(f"\nB={B} N={N} H={H} T={c['T']} E={c['E']}: floors " + "  ".join(f"{k} {v:.2e}" for k, v in fl.items()), end="")
    assert all(v < 2e-6 for v in fl.values()), fl      # K <= 1024 roundings of 2^-24, random signs: far below the 2e-4 cap
    g = gates(fl)
    u = u64(c, seq=True)
    check_u(c, u, u.to(BF), g["u"])
    p, b = grad64(c, seq=True)
    check_grad(c, p, b, g)
    if (B, N, H) in F32_SHAPES:
        f32 = floors(c, f32_operands=True)
        print("   f32 twins " + "  ".join(f"{k} {v:.2e}" for k, v in f32.items()), end="")
        assert all(v < 2e-6 for v in f32.values()), f32
        check_grad(c, *grad64(c, seq=True, f32_operands=True), gates(f32, F32_GATE), f32_operands=True)


@pytest.mark.parametrize("B,N,H", GRID)
def test_the_assertions_bite_u_and_partials(B, N, H):
    c = case(B, N, H)
    T = c["T"]
    g = gates(floors_cpu(B, N, H))
    results = {}

    def grad_fails(**mutant):
        return _fails(check_grad, c, *grad64(c, seq=True, **mutant), g)
    assert not grad_fails()
    if B > 1:
        u = u64(c, seq=True, swap=False)
        assert _fails(check_u, c, u, u.to(BF), g["u"]), "(a) u"
        assert grad_fails(swap=False), "(a) dQ"
        results["a"] = True
    u = u64(c, seq=True)
    assert _fails(check_u, c, u, bf16_trunc(u.double()).to(BF), g["u"]), "bf16 copy of u truncated"
    w = torch.ones(T)
    w[-1] = 0
    assert grad_fails(row_weight=w), "(b)"
    pads = chunks_of(T) * LG_ROWS - T
    if pads:
        w[-1] = 1 + pads
        assert grad_fails(row_weight=w), "(c)"
        results["c"] = True
    assert grad_fails(swap_planes=True), "(d)"
    print(f"\nB={B} N={N} H={H}: mutants (b), (d)" + "".join(f", ({k})" for k in results) + " fail", end="")


@pytest.mark.parametrize("chunks", REDUCE_CHUNKS)
@pytest.mark.parametrize("E", PREP_E)
def test_reduce_and_chain_floors_and_bite(E, chunks):
    fig = {}
    for method, r in (("kadaptation", 32),) + tuple(("lora", r) for r in CHAIN_LORA_R):
        if E != 64 and chunks not in (9, 25) and method == "lora" and r != 8:
            continue                                               # the CPU grid: every rank at E = 64, every E at two chunk counts
        c = chain_case(E, chunks, method, r)
        G = reduced(c)
        for l in range(c["L"]):
            part, db = layer_partial(c, l)
            if method == "lora":
                part = torch.nan_to_num(part)
            kad = method == "kadaptation"
            o = c["p_layer0"] + l * c["p_layer_stride"] + 4 * E
            start = c["grads0"][o:o + E] if kad else torch.zeros(E)          # (LoRA has no bias)
            fl = dict(G=max_rel(reduce32(part), reduce64(part)), bias=max_rel(bias32(db, start), bias64(db, start)))
            assert fl["G"] < 3e-7 and fl["bias"] < 3e-7, fl
            gG, gb = gate_of(fl["G"], F32_GATE), gate_of(fl["bias"], F32_GATE)
            check_reduce(reduce32(part), part, bias32(db, start) if kad else None, db, start, gG, gb)
            if chunks >= 9:
                assert _fails(check_reduce, reduce32(part, skip=8), part, None, db, start, gG, gb), "(f)"
            if kad:
                assert _fails(check_reduce, reduce32(part), part, bias32(db, start, one_plane=True), db, start, gG, gb), "(e)"
            for k, v in fl.items():
                fig[k] = max(fig.get(k, 0.0), v)
        cf = chain_floor(c)
        fig[f"chain[{method},{r}]"] = max(cf.values())
        assert max(cf.values()) < 5e-7, cf
        gate = gate_of(max(cf.values()), F32_GATE)
        G0 = torch.nan_to_num(G)
        chain32 = chain_kadapt32 if method == "kadaptation" else None
        got, got_s, _ = chain_expected(c, G0, dtype=torch.float32, chain=chain32)
        check_chain(c, got, got_s, G0, gate)
        bad, bad_s, _ = chain_expected(c, G0, dq_scale=1.0)
        assert _fails(check_chain, c, bad.float(), bad_s.float(), G0, gate), "(i)"
        if method == "lora":                                       # a NaN of the pad columns reaching the gradients is seen
            leak = got.clone()
            leak[c["p_layer0"] + 1] = float("nan")
            assert _fails(check_chain, c, leak, got_s, G0, gate)
    print(f"\nE={E} chunks={chunks}: floors " + "  ".join(f"{k} {v:.2e}" for k, v in fig.items()) + f"; mutants (e), {'(f), ' if chunks >= 9 else ''}(i) fail", end="")


@pytest.mark.parametrize("l_lo,l_hi", RULE_RANGES)
def test_rule_sum_floor_and_bite(l_lo, l_hi):
    rc = rule_case()
    s, start = rc["scratch"], rc["start"]
    fl = max_rel(rule_sum32(s, start, l_lo, l_hi), rule_sum64(s, start, l_lo, l_hi))
    gate = gate_of(fl, F32_GATE)
    print(f"\nrule_sum [{l_lo}, {l_hi}): floor {fl:.2e}; mutants (g) fail", end="")
    assert fl < 3e-7
    check_rule_sum(rule_sum32(s, start, l_lo, l_hi), s, start, l_lo, l_hi, gate)
    assert _fails(check_rule_sum, rule_sum32(s, start, l_lo, l_hi, miss_lo=True), s, start, l_lo, l_hi, gate), "(g) l_lo missing"
    assert _fails(check_rule_sum, rule_sum32(s, start, l_lo, l_hi, overwrite=True), s, start, l_lo, l_hi, gate), "(g) overwritten"
    poisoned = s.clone()
    poisoned[:l_lo] = float("nan")
    poisoned[l_hi:] = float("nan")
    assert torch.equal(rule_sum32(poisoned, start, l_lo, l_hi), rule_sum32(s, start, l_lo, l_hi))


def test_rule_sum_in_two_ranges_from_the_top_has_the_bits_of_one_call():
    rc = rule_case()
    s, start = rc["scratch"], rc["start"]
    assert torch.equal(rule_sum32(s, rule_sum32(s, start, 12, 24), 0, 12), rule_sum32(s, start, 0, 24))
    assert not torch.equal(rule_sum32(s, rule_sum32(s, start, 0, 12), 12, 24), rule_sum32(s, start, 0, 24))     # the order matters in f32


@pytest.mark.parametrize("E", PREP_E)
def test_prep_floors_and_bite(E):
    cases = [prep_case(E, "kadaptation")] + [prep_case(E, "lora", r) for r in LORA_R]
    for c in cases:
        for f32 in (False, True):
            gate = prep_gates(c, f32)
            fl = prep_floor(c, f32)
            print(f"\nE={E} {c['method']} r={c['r']} {'f32' if f32 else 'bf16'}: floors " + "  ".join(f"{k} {v:.2e}" for k, v in fl.items()), end="")
            for k, v in fl.items():
                assert v <= (1e-7 if (f32 or k == "q32") else 2.0 ** -8), (k, v)      # half a bf16 ulp
            for l in range(c["L"]):
                check_prep(c, l, prep_panels(c, l, f32=f32), f32, gate)
                if not f32:
                    assert _fails(check_prep, c, l, prep_panels(c, l, q=trunc_store), f32, gate), "(j)"
                if c["method"] == "lora" and c["r"] < 32:
                    assert _fails(check_prep, c, l, prep_panels(c, l, f32=f32, dirty_pad=True), f32, gate), "(h)"
                if l:                                              # the panels of another layer: a wrong per-layer advance
                    assert _fails(check_prep, c, l, prep_panels(c, l - 1, f32=f32), f32, gate)
    print(f"\nE={E}: mutants (h), (j) fail", end="")


def kron_H(s, t, ql, qr):
    """the reference model's H = sum_i kron(rule_i, W_i) with rule_i = s_i t_i^T (32 x 32) and W_i = l_i r_i^T (F x F)"""
    return sum(torch.kron(torch.outer(s[i], t[i]), torch.outer(ql[i], qr[i])) for i in range(32))


@pytest.mark.parametrize("E", (64, 128))
def test_kron_definition_equals_the_rank32_panels(E):
    c = prep_case(E, "kadaptation")
    for l in range(c["L"]):
        p = c["layer_params"][l].double()
        ql, qr = p[:E].view(32, E // 32), p[E:2 * E].view(32, E // 32)
        s1, t1, s2, t2 = c["rule"].double()
        Pq, Pv, Qq, Qv = prep_factors(c, l, F64)
        assert max_rel(Pq @ Qq.t(), kron_H(s1, t1, ql, qr)) < 1e-14
        assert max_rel(Pv @ Qv.t(), kron_H(s2, t2, ql, qr)) < 1e-14


@pytest.mark.parametrize("E", (64, 128))
def test_chain_rule_equals_autograd_through_the_kron_definition(E):
    """L = ascale * sum(dDelta_q . (x H_q) + dDelta_v . (x H_v)) with H from kron: autograd's gradients of the six factors equal
    chain_kadapt64 applied to G = (x^T (dDelta_q Q_q), x^T (dDelta_v Q_v), dDelta_q^T (x P_q), dDelta_v^T (x P_v))"""
    g = torch.Generator().manual_seed(E)
    T, F = 37, E // 32
    x, dq, dv = (torch.randn(T, E, generator=g, dtype=F64) for _ in range(3))
    leaves = [torch.randn(32, 32, generator=g, dtype=F64, requires_grad=True) for _ in range(4)] + \
             [torch.randn(32, F, generator=g, dtype=F64, requires_grad=True) for _ in range(2)]
    s1, t1, s2, t2, ql, qr = leaves
    loss = ASCALE * (((x @ kron_H(s1, t1, ql, qr)) * dq).sum() + ((x @ kron_H(s2, t2, ql, qr)) * dv).sum())
    loss.backward()
    with torch.no_grad():
        kr = lambda s, w: (s[:, :, None] * w[:, None, :]).reshape(32, E).t()
        Pq, Pv, Qq, Qv = kr(s1, ql), kr(s2, ql), kr(t1, qr), kr(t2, qr)
        G = torch.stack([x.t() @ (dq @ Qq), x.t() @ (dv @ Qv), dq.t() @ (x @ Pq), dv.t() @ (x @ Pv)])
        d, dl, dr = chain_kadapt64(G, torch.stack([s1, t1, s2, t2]), ql, qr)
        for i, leaf in enumerate((s1, t1, s2, t2)):
            assert max_rel(d[i], leaf.grad) < 1e-12, i
        assert max_rel(dl, ql.grad) < 1e-12 and max_rel(dr, qr.grad) < 1e-12


@pytest.mark.parametrize("struct,cls", [("pevit_lowrank_args", "PevitLowrankArgs"), ("pevit_prep_lowrank_args", "PevitPrepLowrankArgs"),
                                        ("pevit_chain_lowrank_args", "PevitChainLowrankArgs")])
def test_argument_structs_mirror_the_header(struct, cls):
    """the ctypes structures of the test-only entry points name the header's members in the header's order: pointers as pointers,
    size_t, int32_t and float as themselves"""
    import ctypes
    import os
    import re
    from conftest import ROOT
    from pevit_amd import _lib
    src = open(os.path.join(ROOT, "include", "pevit_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
    scalars = {"int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t, "float": ctypes.c_float}
    members = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        kind = decl.split()[0]
        if kind in scalars and "*" not in decl:
            members += [(n.strip(), scalars[kind]) for n in decl[len(kind):].split(",")]
        else:
            assert "*" in decl, decl
            members.append((decl.split("*")[-1].strip(), ctypes.c_void_p))
    assert getattr(_lib, cls)._fields_ == members
    forms = re.search(r"enum pevit_lowrank_form \{(.*?)\}", src, flags=re.S).group(1)
    assert {k.strip().split("=")[0].strip()[len("PEVIT_LOWRANK_"):].lower(): int(k.split("=")[1]) for k in forms.split(",")} == _lib.LOWRANK_FORMS
