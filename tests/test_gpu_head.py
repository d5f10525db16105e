"""The classifier head (csrc/stem_head.hip: bn_fwd_kernel, small_gemm_kernel x 3, ce_loss_kernel, ce_kernel + loss_mean_kernel,
bce_loss_kernel, bn_bwd_kernel), one pevit_launch_head at a time through the test-only pevit_op_head_ex (csrc/verify.hip: it fills
HeadArgs by name, owns no scratch and adds no kernel), at widths and class counts that no engine has.

Inputs, the float64 reference (torch.autograd through F.batch_norm -> F.linear -> F.cross_entropy / BCE-with-logits), the assertions
(`check_head`, `check_identity`) and the gates come from tests/test_head_host.py, which proves on the CPU that they bite (eighteen
wrong heads) and measures the floors.  Forward outputs (ybn, rstd, running statistics, logits): gate = 2 x max(floor, 2^-24), capped by
1e-5 / 1e-6 (running statistics); everything behind the loss keeps the project's gates, 2e-5 max-rel and 1e-5 absolute for the
loss and every row loss.

Every buffer, inputs included, is a window inside a larger allocation whose guard elements before and behind hold a sentinel that must
survive; every output is pre-filled with NaN; gW and gb start from non-zero values and must end at start + gradient; the running
statistics start away from (0, 1); every full launch runs twice from fresh buffers and must give the same bits.

    cross entropy   GRID x {training, eval} x {plain labels, ignore_index rows (row 0 and row B - 1 among them)}
    bad labels      C and -1 at three shapes: NaN in those rows' dlogits, in the loss, gW, gb (and the training-mode dfeat), every
                    other row of dlogits and dybn right
    BCE             multi-hot and soft targets at three shapes
    forms           forward only (nothing behind logits touched); gW null (gb untouched); dfeat null (dybn[0:B] = the row losses,
                    asserted, the rest of dybn untouched)
    alignment       W and feat 4 bytes off a 16-byte boundary: small_gemm_kernel's scalar loads (`vb` false in the logits product)
    identities      (2049, 64, C) with row 2048 ignored == (2048, 64, C) on the first 2048 rows in dlogits, row losses and loss, bit
                    for bit: ce_kernel + loss_mean_kernel against ce_loss_kernel.  Eval mode leaves the running statistics' bits alone.

Figures on the MI355X (max-rel against float64, absolute for the loss; worst over the plain and ignore variants and both modes),
next to the floor of the host emulation (forward outputs) and, in brackets, torch's own float32 head against float64:

    (B, D, C)        ybn               rstd              running mean      running var       logits            | dlogits           gW                gb                dybn              dfeat             loss
    (2,16,1)         1.0e-7 (2.1e-7)   5.5e-8 (1.3e-7)   6.2e-8 (6.1e-8)   7.2e-8 (7.2e-8)   1.4e-7 (2.9e-7)   | 0 [0]             0 [0]             0 [0]             0 [0]             0 [0]             0 [0]
    (7,20,3)         1.3e-7 (1.7e-7)   6.8e-8 (1.4e-7)   8.1e-8 (8.1e-8)   7.9e-8 (7.9e-8)   5.8e-8 (1.5e-7)   | 2.6e-7 [6.1e-8]   2.3e-7 [1.2e-7]   5.6e-7 [1.1e-7]   2.0e-7 [4.7e-8]   2.0e-7 [7.4e-8]   1.3e-7 [3.8e-8]
    (5,6,10)         7.6e-8 (2.0e-7)   2.2e-8 (1.1e-7)   4.0e-8 (4.0e-8)   3.7e-8 (3.7e-8)   8.7e-8 (2.0e-7)   | 7.3e-8 [3.5e-8]   1.5e-7 [6.8e-8]   1.7e-7 [7.5e-8]   1.4e-7 [8.7e-8]   2.8e-7 [1.8e-7]   3.1e-7 [1.2e-7]
    (17,72,63)       1.1e-7 (1.9e-7)   7.5e-8 (1.4e-7)   7.0e-8 (7.0e-8)   4.6e-8 (4.6e-8)   1.3e-7 (2.7e-7)   | 3.5e-7 [4.5e-7]   2.8e-7 [2.9e-7]   1.9e-7 [2.6e-7]   3.1e-7 [4.7e-7]   3.4e-7 [2.8e-7]   3.0e-7 [1.0e-6]
    (16,64,64)       9.8e-8 (1.7e-7)   1.0e-7 (1.5e-7)   5.5e-8 (5.5e-8)   6.0e-8 (6.0e-8)   1.4e-7 (2.8e-7)   | 4.0e-7 [6.8e-7]   5.1e-7 [4.4e-7]   1.2e-7 [1.2e-7]   3.1e-7 [3.0e-7]   2.8e-7 [3.2e-7]   6.4e-7 [6.4e-7]
    (33,64,65)       8.4e-8 (1.5e-7)   8.6e-8 (1.8e-7)   5.4e-8 (5.4e-8)   8.1e-8 (8.1e-8)   1.3e-7 (4.0e-7)   | 4.4e-7 [4.1e-7]   3.3e-7 [2.9e-7]   1.5e-7 [1.9e-7]   3.7e-7 [3.5e-7]   3.8e-7 [4.2e-7]   2.8e-7 [1.3e-7]
    (128,64,127)     1.1e-7 (1.9e-7)   1.1e-7 (1.6e-7)   7.4e-8 (7.4e-8)   9.7e-8 (9.7e-8)   1.9e-7 (5.9e-7)   | 6.4e-7 [6.4e-7]   4.5e-7 [5.9e-7]   2.9e-7 [9.3e-8]   4.9e-7 [5.3e-7]   4.8e-7 [5.3e-7]   6.8e-7 [3.9e-7]
    (129,64,128)     9.4e-8 (1.9e-7)   9.2e-8 (1.6e-7)   5.6e-8 (5.6e-8)   8.5e-8 (7.1e-8)   1.7e-7 (3.6e-7)   | 9.1e-7 [6.7e-7]   3.3e-7 [2.1e-7]   1.3e-7 [9.4e-8]   5.2e-7 [3.8e-7]   5.6e-7 [3.9e-7]   5.8e-7 [4.4e-7]
    (129,64,129)     8.7e-8 (1.7e-7)   1.0e-7 (1.8e-7)   6.7e-8 (6.7e-8)   1.2e-7 (8.9e-8)   1.1e-7 (3.1e-7)   | 5.8e-7 [1.1e-6]   1.5e-7 [2.8e-7]   6.8e-8 [1.1e-7]   3.7e-7 [7.0e-7]   3.5e-7 [7.0e-7]   5.9e-7 [1.0e-7]
    (257,64,100)     9.2e-8 (1.4e-7)   1.1e-7 (1.9e-7)   5.8e-8 (5.8e-8)   8.9e-8 (8.1e-8)   1.3e-7 (4.8e-7)   | 6.9e-7 [7.9e-7]   1.9e-7 [2.1e-7]   6.7e-8 [6.4e-8]   6.2e-7 [6.2e-7]   6.4e-7 [7.6e-7]   7.1e-7 [1.2e-6]
    (128,512,1000)   8.4e-8 (1.6e-7)   1.2e-7 (1.7e-7)   8.2e-8 (8.2e-8)   9.9e-8 (9.9e-8)   2.6e-7 (7.4e-7)   | 2.6e-6 [3.1e-6]   1.2e-6 [8.6e-7]   1.5e-7 [2.1e-7]   1.6e-6 [1.9e-6]   1.6e-6 [1.8e-6]   2.7e-6 [2.7e-6]
    (64,768,397)     1.0e-7 (1.7e-7)   1.2e-7 (1.6e-7)   6.4e-8 (6.4e-8)   8.6e-8 (1.1e-7)   3.6e-7 (1.2e-6)   | 2.7e-6 [5.5e-6]   1.1e-6 [2.6e-6]   2.2e-7 [6.7e-7]   1.5e-6 [3.2e-6]   1.6e-6 [3.2e-6]   3.0e-7 [2.8e-7]
    (2048,64,3)      9.9e-8 (1.6e-7)   1.0e-7 (1.9e-7)   5.1e-8 (5.1e-8)   9.1e-8 (9.1e-8)   1.8e-7 (2.9e-7)   | 5.5e-7 [6.5e-7]   3.2e-7 [1.7e-7]   1.9e-7 [1.9e-7]   4.5e-7 [5.5e-7]   4.4e-7 [5.7e-7]   1.6e-7 [1.6e-7]
    (2049,64,3)      1.2e-7 (1.8e-7)   1.3e-7 (2.2e-7)   7.6e-8 (7.6e-8)   7.3e-8 (7.9e-8)   1.6e-7 (3.2e-7)   | 8.7e-7 [1.1e-6]   2.7e-7 [2.2e-7]   1.7e-7 [1.4e-7]   8.1e-7 [1.1e-6]   9.0e-7 [1.1e-6]   4.3e-7 [4.3e-7]
    (2049,64,130)    9.7e-8 (1.9e-7)   1.4e-7 (1.8e-7)   8.8e-8 (8.8e-8)   9.0e-8 (9.0e-8)   1.1e-7 (2.9e-7)   | 8.2e-7 [1.0e-6]   1.1e-7 [1.6e-7]   3.9e-8 [3.6e-8]   4.5e-7 [5.0e-7]   4.8e-7 [5.7e-7]   7.2e-7 [7.2e-7]
    BCE (multi-hot and soft targets):
    (7,20,3)         logits 5.8e-8  dlogits 1.2e-7  gW 1.5e-7  gb 7.6e-8  dybn 1.7e-7  dfeat 3.4e-7  loss 6.3e-8
    (129,64,129)     logits 1.1e-7  dlogits 3.2e-7  gW 3.9e-8  gb 3.6e-8  dybn 2.0e-7  dfeat 2.4e-7  loss 1.4e-7
    (64,768,397)     logits 3.6e-7  dlogits 4.1e-6  gW 3.2e-8  gb 3.7e-8  dybn 3.4e-7  dfeat 4.7e-7  loss 1.2e-7

    out-of-range labels (C and -1) at (7,20,3), (33,64,65), (129,64,129): NaN exactly in the documented places, the other rows'
    dlogits 5.4e-8 .. 5.8e-7, dybn 5.2e-8 .. 3.5e-7.  Row losses (dfeat null) 1.4e-7 .. 3.0e-6 absolute.  Operands 4 bytes off: the
    figures of the aligned run at (7,20,3); (129,64,128) dlogits 6.5e-7, dfeat 5.6e-7.  Both identities hold bit for bit at C = 3, 130.
    The 89 tests of this file took 3.5 s.
No case failed and no kernel was changed.
"""
import ctypes as C

import pytest
import torch

from test_gpu_kernel_forms import NAN, S, ok, refused, same_bits
from test_head_host import (BAD_GRID, BCE_GRID, BF, FORM_GRID, GRID, IDENTITY_C, OFFSET_GRID, bad_rows, case, check_head, check_identity,
                            identity_pair)
from test_movers_host import sentinel, window

pytestmark = pytest.mark.gpu
GUARD_ROWS = 8


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pevit_amd import _lib
    return _lib.load()


class Win:
    """a [shape] window inside a larger allocation: GUARD_ROWS rows of the sentinel before and behind (`off` more elements before:
    a window that is off its natural alignment)"""

    def __init__(self, shape, dtype=torch.float32, data=None, fill=NAN, off=0):
        init = data.to(dtype) if data is not None else torch.full(tuple(shape), fill, dtype=dtype)
        buf, self.lo = window(init, guard=GUARD_ROWS * (init.numel() // shape[0]), off=off)
        self.base, self.hi = buf.cuda(), self.lo + init.numel()
        self.t = self.base[self.lo:self.hi].view(*shape)
        self.start = self.t.clone()

    def intact(self):
        sent = sentinel(self.base.dtype)
        return bool((self.base[:self.lo] == sent).all()) and bool((self.base[self.hi:] == sent).all())

    def untouched(self):
        return same_bits(self.t, self.start) if self.t.dtype.is_floating_point else torch.equal(self.t, self.start)

    @property
    def ptr(self):
        return self.t.data_ptr()


def launch(lib, c, training, form="full", off=0):
    """one pevit_op_head_ex; returns {name: CPU tensor} of what the form writes.  Asserts the guards and what the form must not touch."""
    from pevit_amd._lib import PevitHeadArgs
    B, D, Cc = c["B"], c["D"], c["C"]
    w = dict(feat=Win((B, D), data=c["feat"], off=off), W=Win((Cc, D), data=c["W"], off=off), bias=Win((Cc,), data=c["bias"]),
             gW=Win((Cc, D), data=c["gW0"]), gb=Win((Cc,), data=c["gb0"]), running_mean=Win((D,), data=c["rm0"]),
             running_var=Win((D,), data=c["rv0"]), ybn=Win((B, D)), rstd=Win((D,)), logits=Win((B, Cc)), dlogits=Win((B, Cc)),
             dybn=Win((B, D)), loss=Win((1,)), dfeat=Win((B, D)), dfeat_bf16=Win((B, D), dtype=BF))
    if c["labels"] is not None:
        w["labels"] = Win((B,), dtype=torch.int64, data=c["labels"])
    if c["targets"] is not None:
        w["targets"] = Win((B, Cc), data=c["targets"])
    absent = {"forward": ("labels", "targets"), "no_gw": ("gW", "gb"), "no_dfeat": ("dfeat", "dfeat_bf16"), "full": ()}[form]
    a = PevitHeadArgs()
    for name, win in w.items():
        if name not in absent or name == "gb":            # (gb is passed without gW: the launcher must not write it)
            setattr(a, name, win.ptr)
    a.training, a.B, a.D, a.Cc = int(training), B, D, Cc
    ok(lib, lib.pevit_op_head_ex(S(), C.byref(a)))
    for name, win in w.items():
        assert win.intact(), f"{name}: a guard element was overwritten"
    for name in ("feat", "W", "bias", "labels", "targets"):
        assert name not in w or w[name].untouched(), name
    out = {k: w[k].t.cpu() for k in ("ybn", "rstd", "logits")}
    out["rm"], out["rv"] = w["running_mean"].t.cpu(), w["running_var"].t.cpu()
    if form == "forward":
        for name in ("dlogits", "dybn", "loss", "gW", "gb", "dfeat", "dfeat_bf16"):
            assert w[name].untouched(), f"{name} touched by the forward-only form"
        return out
    out["dlogits"], out["loss"] = w["dlogits"].t.cpu(), w["loss"].t.cpu().reshape(())
    if form == "no_gw":
        assert w["gW"].untouched() and w["gb"].untouched()
    else:
        out["gW"], out["gb"] = w["gW"].t.cpu(), w["gb"].t.cpu()
    if form == "no_dfeat":
        assert w["dfeat"].untouched() and w["dfeat_bf16"].untouched()
        flat = w["dybn"].t.reshape(-1)
        nrow = B if c["labels"] is not None else 0          # pevit_launch_head: dybn's head is the row-loss scratch of cross entropy
        assert bool(torch.isnan(flat[nrow:]).all()), "dybn written without a d-feature product"
        if nrow:
            out["rowloss"] = flat[:B].cpu()
    else:
        out["dybn"], out["dfeat"], out["dfeat_bf16"] = w["dybn"].t.cpu(), w["dfeat"].t.cpu(), w["dfeat_bf16"].t.cpu()
    return out


def twice(lib, c, training, label, **kw):
    a, b = launch(lib, c, training, **kw), launch(lib, c, training, **kw)
    for k in a:
        assert same_bits(a[k], b[k]), f"{k}: two launches on the same inputs differ"
    return check_head(a, c, training, label)


@pytest.mark.parametrize("variant", ["plain", "ignore"])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B,D,Cc", GRID)
def test_head_cross_entropy(lib, B, D, Cc, training, variant):
    twice(lib, case(B, D, Cc, variant), training, f"CE ({B},{D},{Cc}) {'train' if training else 'eval'} {variant}")


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B,D,Cc", BAD_GRID)
def test_out_of_range_labels_poison_their_rows_and_the_sums_only(lib, B, D, Cc, training):
    c = case(B, D, Cc, "bad")
    out = launch(lib, c, training)
    check_head(out, c, training, f"bad ({B},{D},{Cc}) {'train' if training else 'eval'}")       # NaN exactly where nan_masks says
    rows = bad_rows(c)
    assert bool(torch.isnan(out["dlogits"][rows]).all()) and bool(torch.isfinite(out["dlogits"][~rows]).all())
    assert bool(torch.isnan(out["loss"])) and bool(torch.isnan(out["gW"]).all()) and bool(torch.isnan(out["gb"]).all())
    assert bool(torch.isfinite(out["dybn"][~rows]).all()) and bool(torch.isfinite(out["logits"]).all())
    rl = launch(lib, c, training, form="no_dfeat")
    check_head(rl, c, training)
    assert bool(torch.isnan(rl["rowloss"][rows]).all()) and bool(torch.isfinite(rl["rowloss"][~rows]).all())


@pytest.mark.parametrize("variant", ["multihot", "soft"])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B,D,Cc", BCE_GRID)
def test_head_bce(lib, B, D, Cc, training, variant):
    twice(lib, case(B, D, Cc, variant), training, f"BCE ({B},{D},{Cc}) {'train' if training else 'eval'} {variant}")


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B,D,Cc", FORM_GRID)
def test_forms_write_what_they_own_and_nothing_else(lib, B, D, Cc, training):
    for variant in ("ignore", "soft"):
        c = case(B, D, Cc, variant)
        full = launch(lib, c, training)
        fwd = launch(lib, c, training, form="forward")
        check_head(fwd, c, training)
        no_gw = launch(lib, c, training, form="no_gw")
        check_head(no_gw, c, training)
        no_df = launch(lib, c, training, form="no_dfeat")
        check_head(no_df, c, training, f"row losses ({B},{D},{Cc}) {'train' if training else 'eval'} {variant}")
        assert ("rowloss" in no_df) == (variant == "ignore")
        for other in (fwd, no_gw, no_df):                  # what a form writes does not depend on what else was asked for
            for k in other:
                if k in full:
                    assert same_bits(other[k], full[k]), k


@pytest.mark.parametrize("B,D,Cc", OFFSET_GRID)
def test_operands_off_a_16_byte_boundary_take_the_scalar_loads(lib, B, D, Cc):
    """W and feat start 4 bytes behind a 16-byte boundary: in small_gemm_kernel `vb` (B operand 16-byte aligned) is false for the
    logits product while `va` (ybn) stays true, so one operand of each chunk is gathered with four 4-byte loads; the same gates hold"""
    for training in (True, False):
        c = case(B, D, Cc, "ignore")
        out = launch(lib, c, training, off=1)
        check_head(out, c, training, f"offset ({B},{D},{Cc}) {'train' if training else 'eval'}")


@pytest.mark.parametrize("Cc", IDENTITY_C)
def test_two_kernel_cross_entropy_has_the_bits_of_the_one_workgroup_kernel(lib, Cc):
    big, small = identity_pair(Cc)
    ob, os_ = launch(lib, big, False, form="no_dfeat"), launch(lib, small, False, form="no_dfeat")
    check_identity(ob, os_)
    check_head(ob, big, False)
    check_head(os_, small, False)
    fb, fs = launch(lib, big, False), launch(lib, small, False)
    assert same_bits(fb["dlogits"], ob["dlogits"]) and same_bits(fs["dlogits"], os_["dlogits"])
    assert same_bits(fb["dybn"][:2048], fs["dybn"]) and same_bits(fb["dfeat"][:2048], fs["dfeat"])      # eval mode: rows are independent


def test_head_ex_refuses_before_launching(lib):
    from pevit_amd._lib import PevitHeadArgs
    c = case(7, 20, 3)
    names = ("feat", "W", "running_mean", "running_var", "ybn", "rstd", "logits", "dlogits", "dybn", "loss", "labels", "targets")
    size = max(c["B"] * c["D"], c["B"] * c["C"], c["C"] * c["D"])          # every operand fits: a refusal that regressed stays in bounds
    buf = {n: torch.full((size,), NAN, device="cuda") for n in names}
    buf["labels"] = torch.zeros(c["B"], dtype=torch.int64, device="cuda")
    snap = {n: t.clone() for n, t in buf.items()}

    def args(drop=(), **kw):
        a = PevitHeadArgs()
        for n in names:
            if n not in drop:
                setattr(a, n, buf[n].data_ptr())
        a.training, a.B, a.D, a.Cc = 1, c["B"], c["D"], c["C"]
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    refused(lib, lib.pevit_op_head_ex(S(), None), "null argument struct")
    for k in ("B", "D", "Cc"):
        for v in (0, -3):
            refused(lib, lib.pevit_op_head_ex(S(), C.byref(args(drop=("targets",), **{k: v}))), "head_ex: B=")
    refused(lib, lib.pevit_op_head_ex(S(), C.byref(args())), "labels and targets are both set")
    refused(lib, lib.pevit_op_head_ex(S(), C.byref(args(drop=("targets",), B=1))), "B >= 2")
    for n in ("feat", "W", "running_mean", "running_var", "ybn", "rstd", "logits"):
        refused(lib, lib.pevit_op_head_ex(S(), C.byref(args(drop=("targets", n)))), "are required")
        refused(lib, lib.pevit_op_head_ex(S(), C.byref(args(drop=("targets", "labels", n)))), "are required")
    for n in ("dlogits", "dybn", "loss"):
        refused(lib, lib.pevit_op_head_ex(S(), C.byref(args(drop=("targets", n)))), "a loss needs")
        refused(lib, lib.pevit_op_head_ex(S(), C.byref(args(drop=("labels", n)))), "a loss needs")
    torch.cuda.synchronize()
    for n in names:
        same = torch.equal(buf[n], snap[n]) if n == "labels" else same_bits(buf[n], snap[n])
        assert same, f"{n}: a refused call launched something"
