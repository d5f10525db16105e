"""Host side of tests/test_gpu_movers.py (no GPU): shapes, inputs, expected values and the assertion (`check_window`) of the per-launch
tests of the small exact kernels around the towers -- conv_weight, cls_row, the four im2col kernels (csrc/stem_head.hip), cast_bf16,
transpose_bf16, permute_rows, zero_fill, scale_f32 (csrc/misc.hip), text_embed, text_eot_gather (csrc/text.hip) -- and the evidence
that the assertion can see what it is meant to see.

Everything here is exact.  An expected value is computed in torch float32 in the kernel's operation order (one multiplication by the
scale, one addition of the positional row, the two correctly rounded divisions of the pixel preprocessing) and rounded once,
to nearest even, where the output is bf16.  `check_window` demands the bits of the WHOLE buffer: the payload with its pad columns, and
the guard elements before and behind it, which must still hold the sentinel.  Outputs are pre-filled with NaN by the GPU file, so an
element that a kernel leaves out keeps NaN bits; `*_want` functions take the initial content and return the content after the launch.

The bite (test_mutants_are_seen): the expected-value functions take `mut`, one wrong kernel each, and `check_window` must fail on the
mutant's buffer wherever the mutant differs from the right value at all:
    tail        the n % 4 tail of cast, the bytes % 16 tail of zero, the pad columns of conv_weight dropped
    one_trip    the grid-stride loop of cast / zero stopping after the first trip of 4096 workgroups
    pitch       transpose writing at pitch `rows` instead of `ldd`
    scale_all   transpose scaling every row, not only rows < scaled_rows
    no_swap     permute_rows without the n/b swap
    last_max    the eot gather taking the last maximum
    no_clamp    token ids not clamped (a negative id wraps from the table's end, an id >= V wraps modulo V)
    trunc       truncation instead of round-to-nearest-even in the bf16 stores
"""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_kernel_forms import NAN, SENT

BF, F32 = torch.bfloat16, torch.float32
GRID_CAP = 4096 * 256                        # lanes of the largest grid of cast_bf16 / zero_fill
CAST_N = (1, 3, 4, 7, 1027, GRID_CAP * 4 + 3 * 1024 + 3)
CAST_SCALES = (1.0, 0.125)
ZERO_BYTES = (1, 15, 16, 17, 4101, 16 * (GRID_CAP + 300) + 9)
TRANSPOSE_SHAPES = ((1, 1), (31, 33), (32, 32), (65, 40), (384, 128))
TRANSPOSE_SCALED = (0, 17, 128)
PERMUTE_SHAPES = ((1, 1, 4), (5, 3, 128), (50, 2, 768), (3, 2, 1024), (2, 3, 1028))          # (N, B, E)
SCALE_N = (1, 255, 256, 257, 1000)
CONV_SHAPES = ((3, 12, 64), (5, 588, 640), (128, 768, 768))                                 # (E, K, Kp)
CLS_SHAPES = ((1, 1, 4), (3, 10, 128), (2, 50, 768), (2, 5, 1000))                           # (B, N, E)
IM2COL_SHAPES = ((3, 48, 16), (2, 224, 32), (2, 224, 14))                                   # (B, R, P) of test_im2col
EMBED_SHAPES = ((1, 1, 4, 1), (3, 7, 64, 50), (2, 77, 512, 1000))                            # (S, N, E, V)
EOT_N = (1, 2, 63, 64, 65, 77, 128)
EOT_E = (4, 256, 260, 512)
PIXEL_MEAN, PIXEL_STD = [0.48145466, 0.4578275, 0.40821073], [0.26862954, 0.26130258, 0.27577711]


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def store(v32, f32, mut=None):
    """the kernels' st_store: f32 as it is, or one round-to-nearest-even to bf16"""
    if f32:
        return v32
    if mut == "trunc":
        return (bits(v32) & -65536).view(F32).to(BF)
    return v32.to(BF)


def sentinel(dtype):
    return SENT if dtype.is_floating_point else 249


def window(payload, guard=64, off=0):
    """(buffer, lo): `payload` flattened between two runs of `guard` sentinel elements (`off` more before it: a payload that is off
    its natural alignment); the one guarded-window helper of tests/test_gpu_head.py and tests/test_gpu_movers.py"""
    flat = payload.reshape(-1)
    s = torch.full((guard + off,), sentinel(flat.dtype), dtype=flat.dtype)
    return torch.cat([s, flat, s[:guard]]), guard + off


def check_window(buf, lo, want):
    """the whole buffer has the expected bits: payload (pad columns included) and both guards"""
    n = want.numel()
    assert buf.dtype == want.dtype and buf.numel() >= lo + n
    sent = sentinel(buf.dtype)
    assert bool((buf[:lo] == sent).all()), "the guard before the buffer was overwritten"
    assert bool((buf[lo + n:] == sent).all()), "the guard behind the buffer was overwritten"
    same = bits(buf[lo:lo + n]) == bits(want.reshape(-1))
    assert bool(same.all()), f"{int((~same).sum())} of {n} elements differ, the first at {int((~same).nonzero()[0])}"


# ---------------------------------------------------------------------------------------------------------------- expected values
def cast_want(init, src, scale, f32, mut=None):
    n = src.numel()
    out = init.clone()
    body = n & ~3
    done = min(body, GRID_CAP * 4) if mut == "one_trip" else body
    v = store(src * torch.tensor(scale, dtype=F32), f32, mut)
    out[:done] = v[:done]
    if mut != "tail":
        out[body:n] = v[body:n]
    return out


def zero_want(init_u8, nbytes, mut=None):
    out = init_u8.clone()
    body = nbytes // 16 * 16
    out[:min(body, GRID_CAP * 16) if mut == "one_trip" else body] = 0
    if mut != "tail":
        out[body:nbytes] = 0
    return out


def transpose_want(init, src, ldd, scaled_rows, scale, f32, mut=None):
    """init [cols][ldd]; dst[c][r] = src[r][c] * (r < scaled_rows ? scale : 1)"""
    rows, cols = src.shape
    factor = torch.ones(rows, 1)
    factor[:rows if mut == "scale_all" else scaled_rows] = scale
    v = store((src * factor).T.contiguous(), f32, mut)
    out = init.clone()
    if mut == "pitch":
        out.view(-1)[:rows * cols] = v.reshape(-1)
    else:
        out[:, :rows] = v
    return out


def permute_want(src, N, B, to_internal, mut=None):
    E = src.shape[-1]
    if mut == "no_swap":
        return src.clone()
    if to_internal:
        return src.view(N, B, E).transpose(0, 1).reshape(N * B, E).contiguous()
    return src.view(B, N, E).transpose(0, 1).reshape(N * B, E).contiguous()


def scale_want(init, n, scale):
    out = init.clone()
    out[:n] = init[:n] * torch.tensor(scale, dtype=F32)
    return out


def conv_weight_want(init, w, Kp, f32, mut=None):
    """w [E][K] -> [E][Kp], pad columns +0"""
    E, K = w.shape
    out = init.clone()
    out[:, :K] = store(w, f32, mut)
    if mut != "tail":
        out[:, K:] = 0
    return out


def cls_row_want(init, cls, pos):
    """init [B][N][E]; row 0 of every image = cls + pos[0], the other rows stay"""
    out = init.clone()
    out[:, 0, :] = cls + pos[0]
    return out


def normalize_u8(u8):
    return (u8.float() / 255.0 - torch.tensor(PIXEL_MEAN).view(1, 3, 1, 1)) / torch.tensor(PIXEL_STD).view(1, 3, 1, 1)


def im2col_want(img, P, Kp, f32, mut=None):
    """img (B, 3, R, R) f32 -> [B (R/P)^2][Kp], k = c P P + py P + px, pad columns +0"""
    B, _, R, _ = img.shape
    G, K = R // P, 3 * P * P
    out = torch.zeros(B * G * G, Kp, dtype=F32 if f32 else BF)
    out[:, :K] = store(F.unfold(img, kernel_size=P, stride=P).transpose(1, 2).reshape(B * G * G, K), f32, mut)
    return out


def embed_ids(S, N, V):
    ids = torch.randint(0, V, (S, N), generator=torch.Generator().manual_seed(S * 1000 + N))
    edge = torch.tensor([-5, V, V + 7, 2 ** 40, 0, V - 1])
    flat = ids.view(-1)
    k = min(flat.numel(), edge.numel())
    flat[flat.numel() - k:] = edge[:k]            # (the one-token case keeps -5)
    return ids


def text_embed_want(ids, table, pos, mut=None):
    V = table.shape[0]
    idx = ids.remainder(V) if mut == "no_clamp" else ids.clamp(0, V - 1)
    return (table[idx] + pos[None, :ids.shape[1], :]).reshape(-1, table.shape[1])


def eot_cases(N):
    """{name: ids [N]}: where the largest id sits"""
    base = torch.randint(1, 1000, (N,), generator=torch.Generator().manual_seed(N))
    cases = {}
    for name, where, top in (("last", (N - 1,), 49407), ("ends", (0, N - 1), 49407), ("63|64", (63, 64), 49407), ("64|127", (64, 127), 49407),
                             ("above 2^31", (N // 2, N - 1), 2 ** 31 + 5)):
        if max(where) < N and len(set(where)) == len(where):
            ids = base.clone()
            ids[list(where)] = top
            if name == "above 2^31":
                ids[0] = 2 ** 31 - 1 if N > 2 else ids[0]      # a 32-bit comparison would rank this one above 2^31 + 5
            cases[name] = ids
    cases.setdefault("last", base.clone())
    return cases


def eot_want(ids, x, mut=None):
    """ids [S][N], x [S][N][E] -> x[s][first argmax]"""
    S, N = ids.shape
    top = ids.max(1, keepdim=True).values
    hit = ids == top
    pos = torch.arange(N).expand(S, N)
    first = torch.where(hit, pos, torch.full_like(pos, -1 if mut == "last_max" else N))
    sel = first.max(1).values if mut == "last_max" else first.min(1).values
    return x[torch.arange(S), sel]


# ---------------------------------------------------------------------------------------------------------------- tests
def fails(buf, lo, want):
    with pytest.raises(AssertionError):
        check_window(buf, lo, want)


def test_check_window_sees_payload_and_guards():
    want = store(rnd(5, 8, seed=1), 0)
    buf, lo = window(want)
    check_window(buf, lo, want)
    for i in (0, lo - 1, lo, lo + 39, lo + 40, buf.numel() - 1):
        bad = buf.clone()
        bad[i] = 1.0
        fails(bad, lo, want)
    neg = buf.clone()
    neg[lo] = -neg[lo]
    fails(neg, lo, want)
    zero = torch.zeros(4)
    zb, zlo = window(zero)
    zb[zlo] = -0.0                     # the sign of a zero counts: pad columns are +0 in bits
    fails(zb, zlo, zero)


def test_mutants_are_seen():
    seen = set()

    def bite(name, right, wrong):
        if torch.equal(bits(right), bits(wrong)):
            return
        seen.add(name)
        buf, lo = window(wrong)
        fails(buf, lo, right)
        buf, lo = window(right)
        check_window(buf, lo, right)
    for n in CAST_N:
        src = rnd(n, seed=n % 1000)
        for f32 in (0, 1):
            init = torch.full((n,), NAN, dtype=F32 if f32 else BF)
            for mut in ("tail", "one_trip", "trunc"):
                bite(mut, cast_want(init, src, 0.125, f32), cast_want(init, src, 0.125, f32, mut))
    for nb in ZERO_BYTES:
        init = torch.full((nb + 40,), 249, dtype=torch.uint8)
        for mut in ("tail", "one_trip"):
            bite("zero " + mut, zero_want(init, nb), zero_want(init, nb, mut))
    for rows, cols in TRANSPOSE_SHAPES:
        src = rnd(rows, cols, seed=rows)
        for ldd in (rows, rows + 8):
            for sr in TRANSPOSE_SCALED:
                init = torch.full((cols, ldd), NAN, dtype=BF)
                right = transpose_want(init, src, ldd, sr, 0.125, 0)
                for mut in ("pitch", "scale_all", "trunc"):
                    bite(mut, right, transpose_want(init, src, ldd, sr, 0.125, 0, mut))
    for N, B, E in PERMUTE_SHAPES:
        src = rnd(N * B, E, seed=N)
        for to_internal in (0, 1):
            bite("no_swap", permute_want(src, N, B, to_internal), permute_want(src, N, B, to_internal, "no_swap"))
            assert torch.equal(permute_want(permute_want(src, N, B, 1), N, B, 0), src)
    for E, K, Kp in CONV_SHAPES:
        w = rnd(E, K, seed=E)
        init = torch.full((E, Kp), NAN, dtype=BF)
        for mut in ("tail", "trunc"):
            bite("conv " + mut, conv_weight_want(init, w, Kp, 0), conv_weight_want(init, w, Kp, 0, mut))
    for S, N, E, V in EMBED_SHAPES:
        ids, table, pos = embed_ids(S, N, V), rnd(V, E, seed=V), rnd(N, E, seed=N + 1)
        bite("no_clamp", text_embed_want(ids, table, pos), text_embed_want(ids, table, pos, "no_clamp"))
    for N in EOT_N:
        for name, ids in eot_cases(N).items():
            x = rnd(1, N, 8, seed=N)
            bite("last_max", eot_want(ids[None], x), eot_want(ids[None], x, "last_max"))
    img = rnd(1, 3, 28, 28, seed=2)
    bite("im2col trunc", im2col_want(img, 14, 640, 0), im2col_want(img, 14, 640, 0, "trunc"))
    assert seen == {"tail", "one_trip", "trunc", "zero tail", "zero one_trip", "pitch", "scale_all", "no_swap", "conv tail", "conv trunc",
                    "no_clamp", "last_max", "im2col trunc"}


def test_expected_values_state_their_edges():
    ids = embed_ids(3, 7, 50)
    assert {-5, 50, 57, 2 ** 40} <= set(ids.view(-1).tolist())
    assert int(embed_ids(1, 1, 1)[0, 0]) == -5
    for N in EOT_N:
        cs = eot_cases(N)
        assert "last" in cs
        assert ("ends" in cs) == (N >= 2) and ("63|64" in cs) == (N >= 65) and ("64|127" in cs) == (N >= 128)
        for name, ids in cs.items():
            x = torch.arange(N, dtype=F32).view(1, N, 1).expand(1, N, 4).contiguous()
            assert int(eot_want(ids[None], x)[0, 0]) == int(torch.argmax(ids))         # torch.argmax: the first maximum
    u8 = torch.arange(256, dtype=torch.uint8).repeat(3 * 16 * 16 // 256 * 1, 1).view(1, 3, 16, 16)
    assert normalize_u8(u8).dtype == F32
    assert float(im2col_want(normalize_u8(u8), 16, 832, 1)[:, 768:].abs().sum()) == 0.0
