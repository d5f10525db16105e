"""Kernel-level parity, part 1: HIP kernels called one at a time through the C ABI, against a plain PyTorch
fp32 statement of the same op evaluated on the same (bf16-rounded) operands.

Covered here: the bf16 GEMM family (epilogues 0-8, every tile configuration, the stream-K / k-split / few-row paths), LayerNorm
forward and backward in their plain form (f32 dy, f32 residual gradient, compact rows), the attention core forward and backward at
N in {1, 10, 50, 64, 197, 257} with row pitches equal to the width (the N <= 64 instance and the two compile-time-N forward
instances), delta_add and its fusion with the attention forward, and the low-rank adapter products.
Elsewhere: every GEMM epilogue on every kernel family and operand form, bit for bit on exactly representable operands, with
guarded buffers and pairwise different pitches, in test_gpu_gemm_forms.py (its table, operands and references:
test_gemm_forms_host.py); the other attention token counts (the runtime-N forward instances, the backward kernel's shared last tile, other
pitches), the LayerNorm forms that the training step selects (bf16 dy, the in-place bf16 residual gradient, class-token period and
row stride, column scales, e4m3 copy) and the attention e4m3 copy / class-token-only dO in test_gpu_kernel_forms.py; the post-MLP
adapter kernels, epilogues 9-12, stem, head and SGD in test_gpu_ops2.py; the fp8 kernels in test_gpu_fp8.py; attn_probs in
test_gpu_attention_seam.py and test_gpu_kernel_forms.py; the all-reduce in test_gpu_allreduce.py.

Tolerances: f32 outputs of bf16xbf16 MFMA contractions differ from the torch reference only by
summation order -> 2e-4 relative-to-max; bf16 outputs add one rounding (2^-9) -> 1e-2.
"""
import ctypes as C
import math

import pytest
import torch

from conftest import max_rel, rel_err

pytestmark = pytest.mark.gpu

EPI = dict(QKV=0, BIAS_RESID=1, BIAS_GELU=2, DGELU=3, F32=4, BF16=5, BIAS_BF16=6, PATCH=7, BIAS_RELU=8)


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


def rnd(*shape, scale=1.0, seed=0, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def gemm(lib, epi, A, B, M, N, K, bias=None, resid=None, outf=None, outb=None, outb2=None, aux=None,
         head_stride=0, E=0, H=0, tokens=0, b_rows=None):
    ok(lib, lib.pevit_op_gemm(S(), epi, P(A), A.stride(0), P(B), B.stride(0), b_rows or B.shape[0], M, N, K, P(bias),
                              P(resid), resid.stride(0) if resid is not None else 0, P(outf),
                              outf.stride(0) if outf is not None and outf.dim() == 2 else 64,
                              P(outb), outb.stride(0) if outb is not None and outb.dim() == 2 else 0,
                              P(outb2), outb2.stride(0) if outb2 is not None else 0,
                              P(aux), aux.stride(0) if aux is not None else 0, head_stride, E, H, tokens))
    torch.cuda.synchronize()


@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (300, 136, 128), (6400, 768, 768), (1000, 3072, 768), (515, 768, 3072)])
def test_gemm_f32_and_bf16(lib, M, N, K):
    A = rnd(M, K, seed=1, dtype=torch.bfloat16)
    B = rnd(N, K, seed=2, scale=0.05, dtype=torch.bfloat16)
    ref = A.float() @ B.float().T
    out = torch.full((M, N), float("nan"), device="cuda")
    gemm(lib, EPI["F32"], A, B, M, N, K, outf=out)
    assert max_rel(out.cpu(), ref.cpu()) < 2e-4
    outb = torch.zeros((M, N), dtype=torch.bfloat16, device="cuda")
    gemm(lib, EPI["BF16"], A, B, M, N, K, outb=outb)
    assert max_rel(outb.float().cpu(), ref.cpu()) < 1e-2


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5, 6, 7, 8, 9])
@pytest.mark.parametrize("M,N,K", [(6400, 768, 768), (700, 2368, 256), (257, 136, 64), (1300, 640, 1024)])
def test_gemm_every_tile_config_is_bit_identical(lib, cfg, M, N, K):
    """The tile configurations (4-wave 128x128 / 64x128 / 64x64 / 128x64, 8-wave 256x128 / 256x256 / 320x256 -- the last two on the
    staggered kernel, like 9 = 160x256 on 1 x 8 waves, whose 52 pieces per k-tile do not divide by the 8 loader waves --, and the plain-loop twins of the software-pipelined 4-wave kernels) walk K in the
    same order, so forcing any of them must reproduce the heuristic's result bit for bit -- partial tiles in M and N,
    several tiles per persistent workgroup (M=6400 at 64x64) and the fused epilogues included."""
    A = rnd(M, K, seed=1, dtype=torch.bfloat16)
    B = rnd(N, K, seed=2, scale=0.05, dtype=torch.bfloat16)
    bias = rnd(N, seed=5, scale=0.1)
    resid = rnd(M, N, seed=6)
    ref = A.float() @ B.float().T
    outs = []
    for c in (cfg, -1):
        assert lib.pevit_tune(None, b"gemm_config", c) == 0
        # the heuristic's k-split tile (two wave groups on alternate k-tiles) changes the summation split: close, not equal
        # (test_gemm_streamk_hand_off holds it to the torch product); here the comparison is between plain tilings
        assert lib.pevit_tune(None, b"gemm_ksplit", 0) == 0
        try:
            o1 = torch.full((M, N), float("nan"), device="cuda")
            gemm(lib, EPI["BIAS_RESID"], A, B, M, N, K, bias=bias, resid=resid, outf=o1)
            h = torch.zeros((M, N), dtype=torch.bfloat16, device="cuda"); g = torch.zeros_like(h)
            gemm(lib, EPI["BIAS_GELU"], A, B, M, N, K, bias=bias, outb=h, outb2=g)
        finally:
            lib.pevit_tune(None, b"gemm_config", -1); lib.pevit_tune(None, b"gemm_ksplit", 1)
        outs.append((o1, h, g))
    assert max_rel(outs[0][0].cpu(), (ref + bias + resid).cpu()) < 2e-4
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("M,N,K", [(6400, 768, 3072), (6400, 768, 2368 + 0), (2500, 768, 3072), (6333, 760, 2048), (8224, 1024, 1024),
                                   (3200, 768, 3072), (3111, 768, 768)])     # M = 3200: the 96x128 k-split tile (204 tiles)
def test_gemm_streamk_hand_off(lib, M, N, K):
    """Few-tile long-K products leave the plain tiling: with (almost) one 160x128 tile per CU they run on the 8-wave tile
    whose two wave groups take alternate k-tiles (M = 6400 / 6333), with fewer tiles as stream-K -- the tiles x
    k-iterations space cut into one range per resident workgroup, tiles that span ranges completed through partial slabs in
    HBM (M = 2500).  Both change the summation split, both are deterministic.  Checked against the torch
    product, against the plain tiling (different summation split: close, not equal), for run-to-run bit identity, and
    repeatedly with other kernels in flight and warm caches (stale hand-offs show up only under uneven load)."""
    K = K // 64 * 64
    A = rnd(M, K, seed=1, dtype=torch.bfloat16)
    B = rnd((N + 255) // 256 * 256, K, seed=2, scale=0.05, dtype=torch.bfloat16)
    bias = rnd(N, seed=5, scale=0.1)
    resid = rnd(M, N, seed=6)
    ref = A.float() @ B[:N].float().T
    filler = torch.randn(4096, 4096, device="cuda")

    def run():
        o1 = torch.full((M, N), float("nan"), device="cuda")
        gemm(lib, EPI["BIAS_RESID"], A, B, M, N, K, bias=bias, resid=resid, outf=o1, b_rows=B.shape[0])
        o2 = torch.full((M, N), float("nan"), device="cuda")
        gemm(lib, EPI["F32"], A, B, M, N, K, outf=o2, b_rows=B.shape[0])
        o3 = torch.zeros((M, N), dtype=torch.bfloat16, device="cuda")
        gemm(lib, EPI["BF16"], A, B, M, N, K, outb=o3, b_rows=B.shape[0])
        return o1, o2, o3

    sk = run()
    assert lib.pevit_streamk_error(None, S()) == 0
    # in place on the residual buffer (how the engine calls it): the k-split tile reads its residual values before its k-loop
    r2 = resid.clone()
    gemm(lib, EPI["BIAS_RESID"], A, B, M, N, K, bias=bias, resid=r2, outf=r2, b_rows=B.shape[0])
    assert torch.equal(r2, sk[0])
    assert max_rel(sk[0].cpu(), (ref + bias + resid).cpu()) < 2e-4
    assert max_rel(sk[1].cpu(), ref.cpu()) < 2e-4
    assert max_rel(sk[2].float().cpu(), ref.cpu()) < 1e-2
    assert lib.pevit_tune(None, b"gemm_streamk", 0) == 0 and lib.pevit_tune(None, b"gemm_ksplit", 0) == 0
    try:
        plain = run()
    finally:
        lib.pevit_tune(None, b"gemm_streamk", 1); lib.pevit_tune(None, b"gemm_ksplit", 1)
    assert max_rel(sk[1].cpu(), plain[1].cpu()) < 2e-5
    for it in range(12):
        if it % 3 == 0:
            (filler @ filler).sum()            # other work in flight, caches disturbed
        again = run()
        for a, b in zip(sk, again):
            assert torch.equal(a, b), f"stream-K result changed on repetition {it}"
    assert lib.pevit_streamk_error(None, S()) == 0


def test_gemm_detects_transposes_with_identity(lib):
    """A = I (padded) with an asymmetric B must reproduce B^T exactly (cdna guide: asymmetric check)."""
    K = 128
    A = torch.eye(K, dtype=torch.bfloat16, device="cuda")
    B = (torch.arange(256 * K, device="cuda").reshape(256, K) % 251).to(torch.bfloat16)
    out = torch.zeros((K, 256), device="cuda")
    gemm(lib, EPI["F32"], A, B, K, 256, K, outf=out)
    assert torch.equal(out, B.float().T)


def test_gemm_bias_resid_gelu_dgelu(lib):
    M, N, K = 300, 256, 192
    A = rnd(M, K, seed=3, dtype=torch.bfloat16)
    B = rnd(N, K, seed=4, scale=0.08, dtype=torch.bfloat16)
    bias = rnd(N, seed=5, scale=0.1)
    resid = rnd(M, N, seed=6)
    acc = A.float() @ B.float().T
    out = torch.zeros((M, N), device="cuda")
    gemm(lib, EPI["BIAS_RESID"], A, B, M, N, K, bias=bias, resid=resid, outf=out)
    assert max_rel(out.cpu(), (acc + bias + resid).cpu()) < 2e-4
    # in place on the residual buffer
    r2 = resid.clone()
    gemm(lib, EPI["BIAS_RESID"], A, B, M, N, K, bias=bias, resid=r2, outf=r2)
    assert torch.equal(r2, out)
    h = torch.zeros((M, N), dtype=torch.bfloat16, device="cuda")
    g = torch.zeros((M, N), dtype=torch.bfloat16, device="cuda")
    gemm(lib, EPI["BIAS_GELU"], A, B, M, N, K, bias=bias, outb=h, outb2=g)
    href = (acc + bias).to(torch.bfloat16)
    assert max_rel(h.float().cpu(), href.float().cpu()) < 1e-2
    gref = h.float() * torch.sigmoid(1.702 * h.float())
    assert max_rel(g.float().cpu(), gref.cpu()) < 1e-2
    d = torch.zeros((M, N), dtype=torch.bfloat16, device="cuda")
    gemm(lib, EPI["DGELU"], A, B, M, N, K, outb=d, aux=h)
    s = torch.sigmoid(1.702 * h.float())
    dref = acc * (s * (1 + 1.702 * h.float() * (1 - s)))
    assert max_rel(d.float().cpu(), dref.cpu()) < 1e-2
    o = torch.zeros((M, N), dtype=torch.bfloat16, device="cuda")
    gemm(lib, EPI["BIAS_RELU"], A, B, M, N, K, bias=bias, outb=o)
    assert max_rel(o.float().cpu(), torch.relu(acc + bias).cpu()) < 1e-2


def test_gemm_qkv_head_layout(lib):
    E, H, Ntok, Bt = 128, 2, 10, 30
    T, NQ = Bt * Ntok, 3 * E + 64
    A = rnd(T, E, seed=7, dtype=torch.bfloat16)
    W = torch.zeros((512, E), dtype=torch.bfloat16, device="cuda")
    W[:NQ] = rnd(NQ, E, seed=8, scale=0.1, dtype=torch.bfloat16)
    bias = rnd(3 * E, seed=9, scale=0.1)
    qkv = torch.zeros((3, Bt * H, Ntok, 64), dtype=torch.bfloat16, device="cuda")
    t = torch.zeros((T, 64), device="cuda")
    gemm(lib, EPI["QKV"], A, W, T, NQ, E, bias=bias, outf=t, outb=qkv, head_stride=T * E, E=E, H=H, tokens=Ntok)
    acc = A.float() @ W[:NQ].float().T
    ref = (acc[:, :3 * E] + bias).view(Bt, Ntok, 3, H, 64).permute(2, 0, 3, 1, 4).reshape(3, Bt * H, Ntok, 64)
    assert max_rel(qkv.float().cpu(), ref.cpu()) < 1e-2
    assert max_rel(t.cpu(), acc[:, 3 * E:].cpu()) < 2e-4


def test_gemm_patch_embed(lib):
    E, Ntok, Bt, K = 128, 10, 7, 192
    G2 = Ntok - 1
    A = rnd(Bt * G2, K, seed=10, dtype=torch.bfloat16)
    W = rnd(E, K, seed=11, scale=0.1, dtype=torch.bfloat16)
    pos = rnd(Ntok, E, seed=12)
    x = torch.zeros((Bt * Ntok, E), device="cuda")
    ok(lib, lib.pevit_op_gemm(S(), EPI["PATCH"], P(A), K, P(W), K, E, Bt * G2, E, K, None, P(pos), E, P(x), E, None, 0,
                              None, 0, None, 0, 0, E, 0, Ntok))
    torch.cuda.synchronize()
    ref = torch.zeros((Bt, Ntok, E), device="cuda")
    ref[:, 1:] = (A.float() @ W.float().T).view(Bt, G2, E) + pos[1:]
    assert max_rel(x.view(Bt, Ntok, E).cpu(), ref.cpu()) < 2e-4


@pytest.mark.parametrize("rows,E", [(37, 128), (6400, 768), (257, 1024)])
def test_layernorm_fwd_bwd(lib, rows, E):
    x = rnd(rows, E, seed=1, scale=2.0) + 0.5
    g = 1 + rnd(E, seed=2, scale=0.2); b = rnd(E, seed=3, scale=0.2)
    yb = torch.zeros((rows, E), dtype=torch.bfloat16, device="cuda"); yf = torch.zeros((rows, E), device="cuda")
    mean = torch.zeros(rows, device="cuda"); rstd = torch.zeros(rows, device="cuda")
    ok(lib, lib.pevit_op_ln_fwd(S(), P(x), P(g), P(b), rows, E, P(yb), P(yf), P(mean), P(rstd)))
    torch.cuda.synchronize()
    xr = x.clone().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(xr, (E,), g, b, 1e-5)
    assert max_rel(yf.cpu(), ref.detach().cpu()) < 1e-5
    assert max_rel(yb.float().cpu(), ref.detach().cpu()) < 1e-2
    dy = rnd(rows, E, seed=4); dres = rnd(rows, E, seed=5)
    ref.backward(dy)
    dx = torch.zeros((rows, E), device="cuda"); dxb = torch.zeros((rows, E), dtype=torch.bfloat16, device="cuda")
    ok(lib, lib.pevit_op_ln_bwd(S(), P(dy), P(x), P(mean), P(rstd), P(g), P(dres), P(dx), P(dxb), rows, E))
    torch.cuda.synchronize()
    assert max_rel(dx.cpu(), (xr.grad + dres).cpu()) < 2e-5
    assert max_rel(dxb.float().cpu(), dx.cpu()) < 1e-2


def attn_ref(q, k, v):
    s = torch.einsum("hqd,hkd->hqk", q, k)
    p = torch.softmax(s, dim=-1)
    return torch.einsum("hqk,hkd->hqd", p, v), torch.logsumexp(s, dim=-1)


@pytest.mark.parametrize("Bt,H,N", [(3, 2, 50), (2, 2, 10), (1, 12, 50), (2, 2, 197), (1, 3, 257), (2, 1, 64), (1, 1, 1)])
def test_attention_fwd_bwd(lib, Bt, H, N):
    E = H * 64
    q = rnd(Bt * H, N, 64, seed=1, scale=0.35, dtype=torch.bfloat16)
    k = rnd(Bt * H, N, 64, seed=2, dtype=torch.bfloat16)
    v = rnd(Bt * H, N, 64, seed=3, dtype=torch.bfloat16)
    out = torch.zeros((Bt * N, E), dtype=torch.bfloat16, device="cuda")
    lse = torch.zeros((Bt * H, N), device="cuda")
    ok(lib, lib.pevit_op_attn_fwd(S(), P(q), P(k), P(v), P(out), E, P(lse), Bt, H, N))
    torch.cuda.synchronize()
    qf, kf, vf = (t.float().clone().requires_grad_(True) for t in (q, k, v))
    o_ref, lse_ref = attn_ref(qf, kf, vf)
    o_rows = o_ref.view(Bt, H, N, 64).permute(0, 2, 1, 3).reshape(Bt * N, E)
    assert max_rel(out.float().cpu(), o_rows.detach().cpu()) < 1.5e-2
    assert float((lse - lse_ref.detach()).abs().max()) < 2e-2
    do = rnd(Bt * N, E, seed=4, dtype=torch.bfloat16)
    o_rows.backward(do.float())
    ld = 3 * E + 64
    dqkv = torch.zeros((Bt * N, ld), dtype=torch.bfloat16, device="cuda")
    ok(lib, lib.pevit_op_attn_bwd(S(), P(q), P(k), P(v), P(out), E, P(do), E, P(lse), P(dqkv), ld, Bt, H, N))
    torch.cuda.synchronize()

    def rows(g):
        return g.view(Bt, H, N, 64).permute(0, 2, 1, 3).reshape(Bt * N, E)
    for i, g in enumerate((qf.grad, kf.grad, vf.grad)):
        got = dqkv[:, i * E:(i + 1) * E].float()
        assert rel_err(got.cpu(), rows(g).cpu()) < 2e-2, (i, rel_err(got.cpu(), rows(g).cpu()))
    assert float(dqkv[:, 3 * E:].abs().max()) == 0.0      # the u columns are not touched


def _flat_case(Bt=6, N=10, E=128, seed=0):
    H, T = E // 64, Bt * N
    t = rnd(T, 64, seed=seed + 1)                                   # internal (b*N+n) row order
    q32 = rnd(E, 64, seed=seed + 2, scale=0.3)
    bias = rnd(E, seed=seed + 3, scale=0.2)
    to_ref = lambda x: x.view(Bt, N, -1).permute(1, 0, 2).reshape(T, -1)     # rows rr = n*B+b
    to_int = lambda x: x.view(N, Bt, -1).permute(1, 0, 2).reshape(T, -1)
    return H, T, t, q32, bias, to_ref, to_int


@pytest.mark.parametrize("Bt,N,E", [(6, 10, 128), (5, 50, 256), (128, 50, 768)])
def test_delta_add_flat_reinterpretation(lib, Bt, N, E):
    H, T, t, q32, bias, to_ref, _ = _flat_case(Bt, N, E)
    qb = rnd(Bt * H, N, 64, seed=7, dtype=torch.bfloat16); vb = rnd(Bt * H, N, 64, seed=8, dtype=torch.bfloat16)
    q0, v0 = qb.float().clone(), vb.float().clone()
    q16 = q32.bfloat16()               # the kernel's operand: Q rounded to bf16 (like P and Q^T elsewhere on the path), t in f32
    ok(lib, lib.pevit_op_delta_add(S(), P(qb), P(vb), P(t), P(q16), P(bias), 160.0, Bt, N, E))
    torch.cuda.synchronize()
    tr = to_ref(t)
    dq = (160.0 * tr[:, :32] @ q16.float()[:, :32].T + bias).reshape(Bt * H, N, 64)     # the reference's raw reshape
    dv = (160.0 * tr[:, 32:] @ q16.float()[:, 32:].T + bias).reshape(Bt * H, N, 64)
    assert max_rel(qb.float().cpu(), (q0 + dq).cpu()) < 1e-2
    assert max_rel(vb.float().cpu(), (v0 + dv).cpu()) < 1e-2


@pytest.mark.parametrize("Bt,N,E", [(6, 10, 128), (5, 50, 256), (16, 50, 768)])
def test_lowrank_u_and_grads(lib, Bt, N, E):
    H, T, t, q32, bias, to_ref, to_int = _flat_case(Bt, N, E, seed=20)
    ld = 3 * E + 64
    dqkv = torch.zeros((T, ld), dtype=torch.bfloat16, device="cuda")
    dqkv[:, :3 * E] = rnd(T, 3 * E, seed=30, dtype=torch.bfloat16)
    qT = q32.T.contiguous().to(torch.bfloat16)                      # [64][E]
    u32 = torch.zeros((T, 64), device="cuda")
    ok(lib, lib.pevit_op_lowrank_u(S(), P(dqkv), ld, P(qT), P(u32), C.c_void_p(dqkv.data_ptr() + 3 * E * 2), Bt, H, N, E))
    torch.cuda.synchronize()

    def flat(cols):      # row layout -> head layout -> the reference's (rr, e) view
        return cols.float().view(Bt, N, H, 64).permute(0, 2, 1, 3).reshape(T, E)
    dDq, dDv = flat(dqkv[:, :E]), flat(dqkv[:, 2 * E:3 * E])
    u_ref = torch.cat([dDq @ qT[:32].float().T, dDv @ qT[32:].float().T], dim=1)      # rows rr
    assert max_rel(u32.cpu(), to_int(u_ref).cpu()) < 2e-4
    assert max_rel(dqkv[:, 3 * E:].float().cpu(), to_int(u_ref).cpu()) < 1e-2

    xn = rnd(T, E, seed=31, dtype=torch.bfloat16)
    chunks = lib.pevit_op_lowrank_chunks(T)
    partial = torch.zeros((chunks + 1, 4, E, 32), device="cuda")
    dbp = torch.zeros((chunks, 2, E), device="cuda")
    ok(lib, lib.pevit_op_lowrank_grad(S(), P(xn), E, P(u32), P(dqkv), ld, P(t), P(partial), P(dbp), Bt, H, N, E))
    torch.cuda.synchronize()
    G = partial[:chunks].sum(0)
    tr = to_ref(t)
    # the kernel feeds u and t to the bf16 matrix core: the reference rounds them the same way
    ub, tb = u32.bfloat16().float(), tr.bfloat16().float()
    ref = [xn.float().T @ ub[:, :32], xn.float().T @ ub[:, 32:], dDq.T @ tb[:, :32], dDv.T @ tb[:, 32:]]
    for i in range(4):
        assert max_rel(G[i].cpu(), ref[i].cpu()) < 2e-4, i
    assert max_rel(dbp.sum(0).sum(0).cpu(), (dDq + dDv).sum(0).cpu()) < 2e-4


def test_gemm_streamk_with_the_chip_shared(lib):
    """Stream-K's hand-off assumes its workgroups become resident; under data parallelism the engine switches stream-K off
    (engine.forward_backward_dp), and the fused SGD kernel skips its update if a hand-off ever timed out.  Here the kernel
    itself is run while vendor GEMMs on a second stream occupy the CUs (the situation of an overlapped all-reduce): every
    launch must still produce the bit-identical result without raising the error word -- producers publish the tail of a
    tile before they start anything else, so a consumer only ever waits for work that is already running or done."""
    M, N, K = 2500, 768, 3072
    A = rnd(M, K, seed=1, dtype=torch.bfloat16)
    B = rnd(768, K, seed=2, scale=0.05, dtype=torch.bfloat16)
    bias = rnd(N, seed=5, scale=0.1)
    resid = rnd(M, N, seed=6)
    ref = torch.full((M, N), float("nan"), device="cuda")
    gemm(lib, EPI["BIAS_RESID"], A, B, M, N, K, bias=bias, resid=resid, outf=ref, b_rows=768)
    assert lib.pevit_streamk_error(None, S()) == 0
    side = torch.cuda.Stream()
    big = torch.randn(8192, 8192, device="cuda", dtype=torch.bfloat16)
    for it in range(6):
        with torch.cuda.stream(side):
            for _ in range(4):
                big @ big                                   # ~1 ms each on all 256 CUs
        out = torch.full((M, N), float("nan"), device="cuda")
        for _ in range(5):
            gemm(lib, EPI["BIAS_RESID"], A, B, M, N, K, bias=bias, resid=resid, outf=out, b_rows=768)
            assert torch.equal(out, ref)
    side.synchronize()
    assert lib.pevit_streamk_error(None, S()) == 0


@pytest.mark.parametrize("M,N,K", [(6400, 768, 64), (6400, 768, 128), (6400, 768, 192), (6400, 768, 256), (6400, 768, 320),
                                   (6333, 760, 832), (3200, 768, 3072), (3111, 768, 2368), (12800, 768, 768), (5000, 1024, 512)])
@pytest.mark.parametrize("nl", [8, 2])
def test_gemm_phased_ksplit_tile(lib, M, N, K, nl):
    """The phased k-split kernel (two wave groups take the two halves of every k-tile; 4 LDS stages, exact vmcnt waits) at its
    edges: 1, 2, 3 k-tiles (no steady state: prologue and tail only), 4 and 5 (one and two steady iterations), an odd number of
    k-tiles, ragged M and N, the 96x128 form (M = 3200: 204 tiles), several tiles per workgroup (gemm_ksplit=2: M = 12800 gives
    480 tiles; 5000x1024 gives 256 with a partial last m-tile), and with the requests placed between the MFMAs (nl = 2).
    Every epilogue the step runs on it, against the torch product of the same bf16 operands."""
    A = rnd(M, K, seed=1, dtype=torch.bfloat16)
    B = rnd(N, K, seed=2, scale=0.05, dtype=torch.bfloat16)
    bias = rnd(N, seed=5, scale=0.1)
    resid = rnd(M, N, seed=6)
    ref = A.float() @ B.float().T
    # gemm_big=0: keep the 8-wave tiles away from M = 12800 (the heuristic would take 320x256 there)
    for key, val in ((b"gemm_ksplit", 2), (b"gemm_ksplit_mink", 64), (b"gemm_ksplit_stagger", 2), (b"gemm_kphase_nl", nl), (b"gemm_big", 0)):
        assert lib.pevit_tune(None, key, val) == 0
    try:
        o1 = torch.full((M, N), float("nan"), device="cuda")
        gemm(lib, EPI["BIAS_RESID"], A, B, M, N, K, bias=bias, resid=resid, outf=o1)
        assert lib.pevit_debug_last_gemm_path() == 4, "the heuristic did not take the phased k-split kernel for this shape"
        o2 = torch.full((M, N), float("nan"), device="cuda")
        gemm(lib, EPI["F32"], A, B, M, N, K, outf=o2)
        o3 = torch.zeros((M, N), dtype=torch.bfloat16, device="cuda")
        gemm(lib, EPI["BF16"], A, B, M, N, K, outb=o3)
        # in place on the residual stream, as the block runs it (x += proj(...))
        x = resid.clone()
        gemm(lib, EPI["BIAS_RESID"], A, B, M, N, K, bias=bias, resid=x, outf=x)
    finally:
        for key, val in ((b"gemm_ksplit", 1), (b"gemm_ksplit_mink", 512), (b"gemm_kphase_nl", 8), (b"gemm_big", 1)):
            lib.pevit_tune(None, key, val)
    assert max_rel(o1.cpu(), (ref + bias + resid).cpu()) < 2e-4
    assert max_rel(o2.cpu(), ref.cpu()) < 2e-4
    assert max_rel(o3.float().cpu(), ref.cpu()) < 1e-2
    assert torch.equal(x, o1)


@pytest.mark.parametrize("M,N,K", [(3200, 768, 3072), (3111, 768, 2368), (3200, 768, 2048), (3200, 760, 3072)])
def test_gemm_two_k_slices_per_tile(lib, M, N, K):
    """gemm_kphase_kernel<..., KZ> (round 5): where 160x128 tiles fill at most half the chip (batch 64: M = 3200, N = 768) and K is
    long, TWO workgroups share a tile, half of the k-tiles each; the one that arrives last adds the other's partial (stream-K
    workspace, one ticket per tile) and runs the epilogue.  Every epilogue the step runs on it against the torch product; an odd
    number of k-tiles (K = 2368: 18 + 19), the shortest slices the heuristic admits (K = 2048), ragged M and N; launched three times
    (the tickets must be back at zero) with bit-identical results (two slices: the sum does not depend on who arrives last); and
    against the one-workgroup-per-tile form of the same shapes to f32 summation order."""
    A = rnd(M, K, seed=1, dtype=torch.bfloat16)
    B = rnd(N, K, seed=2, scale=0.05, dtype=torch.bfloat16)
    bias = rnd(N, seed=5, scale=0.1)
    resid = rnd(M, N, seed=6)
    ref = A.float() @ B.float().T
    outs = []
    assert lib.pevit_tune(None, b"gemm_kz2", 1) == 0          # opt-in: measured slower than the 96x128 tiles it replaces (gemm.hip)
    try:
        for rep in range(3):
            o1 = torch.full((M, N), float("nan"), device="cuda")
            gemm(lib, EPI["BIAS_RESID"], A, B, M, N, K, bias=bias, resid=resid, outf=o1)
            assert lib.pevit_debug_last_gemm_path() == 7, "the heuristic did not take the two-slice form for this shape"
            o2 = torch.full((M, N), float("nan"), device="cuda")
            gemm(lib, EPI["F32"], A, B, M, N, K, outf=o2)
            o3 = torch.zeros((M, N), dtype=torch.bfloat16, device="cuda")
            gemm(lib, EPI["BF16"], A, B, M, N, K, outb=o3)
            assert lib.pevit_debug_last_gemm_path() == 7
            x = resid.clone()
            gemm(lib, EPI["BIAS_RESID"], A, B, M, N, K, bias=bias, resid=x, outf=x)      # in place on the residual stream
            outs.append((o1, o2, o3, x))
    finally:
        lib.pevit_tune(None, b"gemm_kz2", 0)
    p2 = torch.full((M, N), float("nan"), device="cuda")
    gemm(lib, EPI["F32"], A, B, M, N, K, outf=p2)
    assert lib.pevit_debug_last_gemm_path() != 7
    o1, o2, o3, x = outs[0]
    assert max_rel(o1.cpu(), (ref + bias + resid).cpu()) < 2e-4
    assert max_rel(o2.cpu(), ref.cpu()) < 2e-4
    assert max_rel(o3.float().cpu(), ref.cpu()) < 1e-2
    assert max_rel(o2.cpu(), p2.cpu()) < 1e-5
    assert torch.equal(x, o1)
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)
    assert lib.pevit_streamk_error(None, S()) == 0


@pytest.mark.parametrize("M,N,K,slices", [(128, 768, 3072, 0), (64, 768, 3072, 0), (128, 768, 3072, 2), (128, 768, 3072, 6), (128, 768, 3072, 1),
                                          (100, 512, 1600, 0), (1, 768, 2048, 3), (128, 760, 1536, 5), (37, 1024, 4096, 0)])
def test_gemm_few_row_split_k(lib, M, N, K, slices):
    """Few-row long-K products (c_proj forward / c_fc backward on the class-token rows of the last block) on gemm_skinny_kernel:
    128x64 tiles, 2-6 K slices with a four-stage ring (slices of 4 to 48 k-tiles here, an odd count and a short last slice
    included; one slice = no hand-off at all), the last arriver of a tile adds the partial slabs in slice order.  Every epilogue
    the step runs on it against the torch product; launched twice (the tickets must be back at zero) with bit-identical results
    (fixed summation order, whoever arrives last); strided A rows like the class-token view of a [B][N][E] buffer."""
    assert lib.pevit_tune(None, b"gemm_skinny_slices", slices) == 0
    A = rnd(M, K, seed=1, dtype=torch.bfloat16)
    B = rnd(N, K, seed=2, scale=0.05, dtype=torch.bfloat16)
    bias = rnd(N, seed=5, scale=0.1)
    resid = rnd(M, N, seed=6)
    acc = A.float() @ B.float().T
    outs = []
    for rep in range(2):
        o1 = torch.full((M, N), float("nan"), device="cuda")
        gemm(lib, EPI["BIAS_RESID"], A, B, M, N, K, bias=bias, resid=resid, outf=o1)
        assert lib.pevit_debug_last_gemm_path() == 6, "the heuristic did not take the few-row kernel for this shape"
        o2 = torch.full((M, N), float("nan"), device="cuda")
        gemm(lib, EPI["F32"], A, B, M, N, K, outf=o2)
        o3 = torch.zeros((M, N), dtype=torch.bfloat16, device="cuda")
        gemm(lib, EPI["BF16"], A, B, M, N, K, outb=o3)
        h = torch.zeros((M, N), dtype=torch.bfloat16, device="cuda"); g = torch.zeros_like(h)
        gemm(lib, EPI["BIAS_GELU"], A, B, M, N, K, bias=bias, outb=h, outb2=g)
        d = torch.zeros((M, N), dtype=torch.bfloat16, device="cuda")
        gemm(lib, EPI["DGELU"], A, B, M, N, K, outb=d, aux=h)
        assert lib.pevit_debug_last_gemm_path() == 6
        outs.append((o1, o2, o3, h, g, d))
    o1, o2, o3, h, g, d = outs[0]
    assert max_rel(o1.cpu(), (acc + bias + resid).cpu()) < 2e-4
    assert max_rel(o2.cpu(), acc.cpu()) < 2e-4
    assert max_rel(o3.float().cpu(), acc.cpu()) < 1e-2
    assert max_rel(h.float().cpu(), (acc + bias).cpu()) < 1e-2
    assert max_rel(g.float().cpu(), (h.float() * torch.sigmoid(1.702 * h.float())).cpu()) < 1e-2
    s = torch.sigmoid(1.702 * h.float())
    assert max_rel(d.float().cpu(), (acc * (s * (1 + 1.702 * h.float() * (1 - s)))).cpu()) < 1e-2
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # rows three "tokens" apart, as the class-token rows of a [M][3][K] buffer
    wide = rnd(M, 3 * K, seed=7, dtype=torch.bfloat16)
    As = wide[:, :K]
    o4 = torch.full((M, N), float("nan"), device="cuda")
    gemm(lib, EPI["F32"], As, B, M, N, K, outf=o4)
    assert lib.pevit_debug_last_gemm_path() == 6
    assert max_rel(o4.cpu(), (As.float() @ B.float().T).cpu()) < 2e-4
    # the plain tiling of the same product agrees to summation order
    assert lib.pevit_tune(None, b"gemm_skinny", 0) == 0
    try:
        o5 = torch.full((M, N), float("nan"), device="cuda")
        gemm(lib, EPI["F32"], A, B, M, N, K, outf=o5)
        assert lib.pevit_debug_last_gemm_path() != 6
    finally:
        lib.pevit_tune(None, b"gemm_skinny", 1)
    assert max_rel(o5.cpu(), o2.cpu()) < 2e-4
    lib.pevit_tune(None, b"gemm_skinny_slices", 0)


@pytest.mark.parametrize("Bt,N,E,with_bias", [(6, 10, 128, True), (5, 10, 128, False), (3, 50, 768, True), (128, 50, 768, True),
                                              (64, 50, 768, False), (1, 2, 768, True)])
def test_attn_fwd_delta_is_bit_identical_to_delta_add_then_attn_fwd(lib, Bt, N, E, with_bias):
    """attn_delta.hip: the adapter delta of the raw reshape (model.py:796-799) and the attention core (model.py:806-812) as ONE
    launch, a run of six heads per workgroup (with N = 50, H = 12: exactly 25 reference rows).  Same products in the same order
    and the same roundings as delta_add followed by attn_fwd: q', v', the attention output and the log-sum-exp agree bit for
    bit -- including runs that start inside the batch, a last run with fewer heads (B*H = 10), two tokens per image and LoRA's
    bias-free form."""
    H, T, t, q32, bias, to_ref, _ = _flat_case(Bt, N, E, seed=40)
    if not with_bias:
        bias = None
    assert lib.pevit_op_attn_delta_hpw(Bt, H, N) == 6
    q = rnd(Bt * H, N, 64, seed=41, scale=0.35, dtype=torch.bfloat16)
    k = rnd(Bt * H, N, 64, seed=42, dtype=torch.bfloat16)
    v = rnd(Bt * H, N, 64, seed=43, dtype=torch.bfloat16)
    q1, v1 = q.clone(), v.clone()
    out1 = torch.zeros((Bt * N, E), dtype=torch.bfloat16, device="cuda"); lse1 = torch.zeros((Bt * H, N), device="cuda")
    q16 = q32.bfloat16()
    ok(lib, lib.pevit_op_delta_add(S(), P(q1), P(v1), P(t), P(q16), P(bias), 160.0, Bt, N, E))
    ok(lib, lib.pevit_op_attn_fwd(S(), P(q1), P(k), P(v1), P(out1), E, P(lse1), Bt, H, N))
    q2, v2 = q.clone(), v.clone()
    out2 = torch.zeros_like(out1); lse2 = torch.zeros_like(lse1)
    ok(lib, lib.pevit_op_attn_fwd_delta(S(), P(q2), P(k), P(v2), P(t), P(q16), P(bias), 160.0, P(out2), E, P(lse2), Bt, H, N))
    torch.cuda.synchronize()
    assert not torch.equal(q1, q) and not torch.equal(v1, v)            # the delta is not a no-op in this case
    assert torch.equal(q2, q1) and torch.equal(v2, v1)
    assert torch.equal(out2, out1) and torch.equal(lse2, lse1)
    # ... and against the reference arithmetic (the raw reshape in f32, then softmax attention)
    tr = to_ref(t)
    b0 = bias if bias is not None else torch.zeros(E, device="cuda")
    dq = (160.0 * tr[:, :32] @ q16.float()[:, :32].T + b0).reshape(Bt * H, N, 64)
    dv = (160.0 * tr[:, 32:] @ q16.float()[:, 32:].T + b0).reshape(Bt * H, N, 64)
    assert max_rel(q2.float().cpu(), (q.float() + dq).cpu()) < 1e-2
    o_ref, _ = attn_ref(q2.float(), k.float(), v2.float())
    o_rows = o_ref.view(Bt, H, N, 64).permute(0, 2, 1, 3).reshape(Bt * N, E)
    assert max_rel(out2.float().cpu(), o_rows.cpu()) < 1.5e-2


def test_attn_delta_geometries():
    """Which towers take the fused form: six heads must start on a reference-row boundary (6*N % H == 0) and span at most 32
    reference rows.  ViT-B/32 (N = 50, H = 12) does; ViT-B/16 (N = 197) and ViT-L/14 (N = 257, H = 16) keep the two kernels."""
    from pevit_amd import _lib
    lib = _lib.load()
    assert lib.pevit_op_attn_delta_hpw(128, 12, 50) == 6 and lib.pevit_op_attn_delta_hpw(64, 12, 50) == 6
    assert lib.pevit_op_attn_delta_hpw(64, 12, 197) == 0 and lib.pevit_op_attn_delta_hpw(32, 16, 257) == 0
    assert lib.pevit_op_attn_delta_hpw(5, 4, 50) == 0          # 75 reference rows per run: more than two 16-row groups
