"""The small exact kernels around the towers, one launch at a time through the test-only pass-throughs of csrc/verify.hip
(pevit_op_cast_ex, pevit_op_zero, pevit_op_transpose, pevit_op_permute_rows, pevit_op_scale_f32, pevit_op_conv_weight,
pevit_op_cls_row, pevit_op_im2col_ex, pevit_op_text_embed, pevit_op_text_eot_gather): until now only whole towers ran them, at the
towers' sizes.  Shapes, expected values and the assertion come from tests/test_movers_host.py, which shows on the CPU that the
assertion sees eight kinds of wrong kernel.

Every check is bit identity of the whole buffer: outputs are pre-filled with NaN and sit between two guards of 64 sentinel elements;
the expected content is computed in torch float32 in the kernel's operation order and rounded once to bf16 where the output is bf16;
pad columns are +0 in bits.  Both storages (bf16 and the f32 of the verification mode) run wherever the launcher takes the flag.

    cast         n = 1, 3, 4, 7, 1027 and 4096*256*4 + 3*1024 + 3 (the 4096-workgroup cap, a second grid-stride trip and an n % 4 tail)
    zero         1, 15, 16, 17, 4101 and 16*(4096*256 + 300) + 9 bytes of a sentinel-filled buffer; a pointer 4 bytes off is refused
    transpose    five shapes, ldd = rows and rows + 8, scaled_rows 0 / 17 / 128 (inside a tile, at a tile edge)
    permute_rows E up to 1028 (a second trip of the 192 lanes), both directions, the round trip; E = 6 refused
    scale_f32    n around the 256-lane workgroup; the element behind n survives
    conv_weight, cls_row, the four im2col kernels in both storages, text_embed with clamped ids, text_eot_gather with the first maximum

On the MI355X every buffer of the 70 tests had the expected bits (0.9 s in all).  No case failed and no kernel was changed.
"""
import ctypes as C

import pytest
import torch

from test_gpu_kernel_forms import NAN, SENT, S, ok, refused
from test_movers_host import (BF, CAST_N, CAST_SCALES, CLS_SHAPES, CONV_SHAPES, EMBED_SHAPES, EOT_E, EOT_N, F32, IM2COL_SHAPES,
                              PERMUTE_SHAPES, PIXEL_MEAN, PIXEL_STD, SCALE_N, TRANSPOSE_SCALED, TRANSPOSE_SHAPES, ZERO_BYTES,
                              cast_want, check_window, cls_row_want, conv_weight_want, embed_ids, eot_cases, eot_want, im2col_want,
                              normalize_u8, permute_want, rnd, scale_want, text_embed_want, transpose_want, window, zero_want)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pevit_amd import _lib
    return _lib.load()


class Dev:
    """`init` on the GPU between two guards; .p = pointer to the payload; .check(want) = bits of the whole buffer"""

    def __init__(self, init):
        buf, self.lo = window(init)
        self.buf = buf.cuda()
        self.p = C.c_void_p(self.buf.data_ptr() + self.lo * self.buf.element_size())

    def check(self, want):
        torch.cuda.synchronize()
        check_window(self.buf.cpu(), self.lo, want)


def nans(*shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype)


def dt(f32):
    return F32 if f32 else BF


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("n", CAST_N)
def test_cast(lib, n, f32):
    src = rnd(n, seed=n % 1000)
    s = Dev(src)
    for scale in CAST_SCALES:
        out = Dev(nans(n, dtype=dt(f32)))
        ok(lib, lib.pevit_op_cast_ex(S(), s.p, out.p, n, scale, f32))
        out.check(cast_want(nans(n, dtype=dt(f32)), src, scale, f32))
    s.check(src)
    if not f32:                       # the production entry point is the same launch
        out = Dev(nans(n, dtype=BF))
        ok(lib, lib.pevit_op_cast_bf16(S(), s.p, out.p, n, 0.125))
        out.check(cast_want(nans(n, dtype=BF), src, 0.125, 0))


@pytest.mark.parametrize("nbytes", ZERO_BYTES)
def test_zero(lib, nbytes):
    init = torch.full((nbytes + 40,), 249, dtype=torch.uint8)
    d = Dev(init)
    ok(lib, lib.pevit_op_zero(S(), d.p, nbytes))
    d.check(zero_want(init, nbytes))
    ok(lib, lib.pevit_op_zero(S(), d.p, 0))
    refused(lib, lib.pevit_op_zero(S(), C.c_void_p(d.p.value + 4), 16), "16-byte aligned")
    d.check(zero_want(init, nbytes))


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("rows,cols", TRANSPOSE_SHAPES)
def test_transpose(lib, rows, cols, f32):
    src = rnd(rows, cols, seed=rows)
    s = Dev(src)
    for ldd in (rows, rows + 8):
        for scaled in TRANSPOSE_SCALED:
            init = nans(cols, ldd, dtype=dt(f32))
            out = Dev(init)
            ok(lib, lib.pevit_op_transpose(S(), s.p, rows, cols, out.p, ldd, scaled, 0.125, f32))
            out.check(transpose_want(init, src, ldd, scaled, 0.125, f32))


@pytest.mark.parametrize("N,B,E", PERMUTE_SHAPES)
def test_permute_rows(lib, N, B, E):
    src = rnd(N * B, E, seed=N)
    s = Dev(src)
    for to_internal in (1, 0):
        out = Dev(nans(N * B, E))
        ok(lib, lib.pevit_op_permute_rows(S(), s.p, out.p, N, B, E, to_internal))
        out.check(permute_want(src, N, B, to_internal))
        back = Dev(nans(N * B, E))
        ok(lib, lib.pevit_op_permute_rows(S(), out.p, back.p, N, B, E, 1 - to_internal))
        back.check(src)
    s.check(src)
    out = Dev(nans(4, 6))
    refused(lib, lib.pevit_op_permute_rows(S(), s.p, out.p, 2, 2, 6, 1), "multiple of 4")
    out.check(nans(4, 6))


@pytest.mark.parametrize("n", SCALE_N)
def test_scale_f32(lib, n):
    init = rnd(n + 3, seed=n)
    d = Dev(init)
    ok(lib, lib.pevit_op_scale_f32(S(), d.p, n, 0.3))
    d.check(scale_want(init, n, 0.3))
    ok(lib, lib.pevit_op_scale_f32(S(), d.p, 0, 0.3))
    d.check(scale_want(init, n, 0.3))


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("E,K,Kp", CONV_SHAPES)
def test_conv_weight(lib, E, K, Kp, f32):
    w = rnd(E, K, seed=E)
    init = nans(E, Kp, dtype=dt(f32))
    out, src = Dev(init), Dev(w)
    ok(lib, lib.pevit_op_conv_weight(S(), src.p, out.p, E, K, Kp, f32))
    out.check(conv_weight_want(init, w, Kp, f32))


@pytest.mark.parametrize("B,N,E", CLS_SHAPES)
def test_cls_row(lib, B, N, E):
    cls, pos = rnd(E, seed=1), rnd(N, E, seed=2)
    init = torch.full((B, N, E), SENT)
    init[:, 0, :] = NAN
    x = Dev(init)
    c, p = Dev(cls), Dev(pos)
    ok(lib, lib.pevit_op_cls_row(S(), c.p, p.p, x.p, B, N, E))
    x.check(cls_row_want(init, cls, pos))


@pytest.mark.parametrize("f32", [0, 1])
@pytest.mark.parametrize("u8", [0, 1])
@pytest.mark.parametrize("B,R,Pp", IM2COL_SHAPES)
def test_im2col(lib, B, R, Pp, u8, f32):
    """im2col8_kernel / im2col_kernel (f32 pixels, against F.unfold) and im2col8_u8_kernel / im2col_u8_kernel (uint8 pixels, against the
    host preprocessing), each in both storages"""
    K = 3 * Pp * Pp
    Kp = (K + 63) // 64 * 64
    G = R // Pp
    if u8:
        pix = torch.randint(0, 256, (B, 3, R, R), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
        img = normalize_u8(pix)
    else:
        pix = img = rnd(B, 3, R, R, seed=1)
    src = Dev(pix)
    out = Dev(nans(B * G * G, Kp, dtype=dt(f32)))
    mean, std = (C.c_float * 3)(*PIXEL_MEAN), (C.c_float * 3)(*PIXEL_STD)
    ok(lib, lib.pevit_op_im2col_ex(S(), src.p, u8, C.cast(mean, C.c_void_p), C.cast(std, C.c_void_p), out.p, B, R, Pp, Kp, f32))
    out.check(im2col_want(img, Pp, Kp, f32))
    src.check(pix)


@pytest.mark.parametrize("S_,N,E,V", EMBED_SHAPES)
def test_text_embed(lib, S_, N, E, V):
    ids, table, pos = embed_ids(S_, N, V), rnd(V, E, seed=V), rnd(N, E, seed=N + 1)
    out = Dev(nans(S_ * N, E))
    i, t, p = Dev(ids), Dev(table), Dev(pos)
    ok(lib, lib.pevit_op_text_embed(S(), i.p, t.p, p.p, out.p, S_, N, E, V))
    out.check(text_embed_want(ids, table, pos))
    for bad in ((0, N, E, V), (S_, 0, E, V), (S_, N, E + 2, V), (S_, N, 0, V), (S_, N, E, 0)):
        refused(lib, lib.pevit_op_text_embed(S(), i.p, t.p, p.p, out.p, *bad), "text_embed: bad shape")
    refused(lib, lib.pevit_op_text_embed(S(), None, t.p, p.p, out.p, S_, N, E, V), "null argument")
    out.check(text_embed_want(ids, table, pos))


@pytest.mark.parametrize("N", EOT_N)
def test_text_eot_gather(lib, N):
    cs = eot_cases(N)
    ids = torch.stack(list(cs.values()))
    S_ = ids.shape[0]
    i = Dev(ids)
    for E in EOT_E:
        x = rnd(S_, N, E, seed=E)
        out = Dev(nans(S_, E))
        xd = Dev(x)
        ok(lib, lib.pevit_op_text_eot_gather(S(), i.p, xd.p, out.p, S_, N, E))
        out.check(eot_want(ids, x))
    refused(lib, lib.pevit_op_text_eot_gather(S(), i.p, xd.p, out.p, 1, 129, 4), "text_eot_gather: bad shape")
    refused(lib, lib.pevit_op_text_eot_gather(S(), i.p, xd.p, out.p, 1, N, 6), "text_eot_gather: bad shape")
    refused(lib, lib.pevit_op_text_eot_gather(S(), i.p, None, out.p, 1, N, 4), "null argument")
    out.check(eot_want(ids, x))
