"""CPU-side checks of the activation workspace's size and of the one part of it that carries state between launches.

``pevit_bind`` compares the caller's buffer with ``pevit_workspace_bytes(ctx, max_batch)`` only, and every call carves the buffer
afresh for ITS batch (``layout_workspace`` in csrc/ctx.hip): a batch below ``max_batch`` must never need more bytes than
``max_batch`` itself, for every method, every weight format ``pevit_ctx_create`` takes, and a text context (whose workspace is the
inference layout).  Several terms of the layout are not linear in the batch -- the per-chunk partials of the adapter gradients
(``pevit_lowrank_chunks``, ``pevit_tn_chunks``, the LayerNorm-affine blocks) -- so this is checked batch by batch, 1 to 130.

``pevit_workspace_state_bytes`` is the prefix tests/test_gpu_workspace.py leaves alone when it overwrites the workspace: it must
be the stream-K flag region of csrc/kernels.h (flags + error word + skipped-update counter), the same for every context, and
smaller than every workspace."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

from pevit_amd import _lib
from pevit_amd.synth import ARCHS

METHODS = ["kadaptation", "lora", "adapter", "compacter", "none"]
FORMATS = ["bf16", "fp8", "fp8-act", "f32-verify"]
TINY = ["tiny-128", "tiny-256", "tiny-n257"]
BATCHES = range(1, 131)


def creatable(method, weight_format):
    """fp8 weights exist for the attention-site methods and the frozen tower only (pevit_ctx_create)"""
    return not (weight_format in ("fp8", "fp8-act") and method in ("adapter", "compacter"))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def image_ctx(lib, arch_name, method, weight_format):
    a = ARCHS[arch_name]
    d = _lib.PevitDims(a.width, a.layers, a.patch, a.resolution, a.embed_dim, _lib.METHOD_IDS[method], 4, 10,
                       _lib.WEIGHT_FORMATS[weight_format])
    ctx = C.c_void_p()
    return lib.pevit_ctx_create(C.byref(d), C.byref(ctx)), ctx


# (width, layers, context_length, vocab_size, out_dim): the tiny text tower of tests/golden/text_w128_l2_n8.json and CLIP's own
TEXT_TOWERS = {"text-w128_l2_n8": (128, 2, 8, 32, 64), "text-w512_l12_n77": (512, 12, 77, 49408, 512)}


def text_ctx(lib, tower, weight_format):
    d = _lib.PevitTextDims(*TEXT_TOWERS[tower], _lib.WEIGHT_FORMATS[weight_format])
    ctx = C.c_void_p()
    return lib.pevit_text_create(C.byref(d), C.byref(ctx)), ctx


def flag_region_of_the_sources():
    """(PEVIT_SK_MAX_SLOTS + 2) * 4 with the slot count read from csrc/kernels.h"""
    src = open(os.path.join(ROOT, "pevit_amd", "csrc", "kernels.h")).read()
    return (int(re.search(r"constexpr int PEVIT_SK_MAX_SLOTS = (\d+);", src).group(1)) + 2) * 4


def check_sizes(lib, ctx):
    state = lib.pevit_workspace_state_bytes(ctx)
    assert state == flag_region_of_the_sources()
    sizes = [lib.pevit_workspace_bytes(ctx, B) for B in BATCHES]
    assert sizes[0] > state                                 # there is scratch behind the prefix even for one image
    for B, (lo, hi) in zip(BATCHES, zip(sizes, sizes[1:])):
        assert lo <= hi, f"batch {B} needs {lo} bytes, batch {B + 1} only {hi}: a workspace bound for {B + 1} is too small for {B}"
    assert all(s % 256 == 0 for s in sizes)                 # every slot starts 256-byte aligned, the end included
    assert lib.pevit_workspace_bytes(ctx, 0) == 0 and lib.pevit_workspace_bytes(ctx, -3) == 0


@pytest.mark.parametrize("weight_format", FORMATS)
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("arch_name", TINY + ["ViT-B/32"])
def test_a_smaller_batch_never_needs_a_larger_workspace(lib, arch_name, method, weight_format):
    rc, ctx = image_ctx(lib, arch_name, method, weight_format)
    if not creatable(method, weight_format):
        assert rc != 0 and b"fp8 weights are built for" in lib.pevit_last_error()
        return
    assert rc == 0, lib.pevit_last_error()
    try:
        check_sizes(lib, ctx)
    finally:
        lib.pevit_ctx_destroy(ctx)


@pytest.mark.parametrize("weight_format", ["bf16", "f32-verify"])
@pytest.mark.parametrize("tower", sorted(TEXT_TOWERS))
def test_text_context_workspace_grows_with_the_prompts(lib, tower, weight_format):
    rc, ctx = text_ctx(lib, tower, weight_format)
    assert rc == 0, lib.pevit_last_error()
    try:
        check_sizes(lib, ctx)
    finally:
        lib.pevit_ctx_destroy(ctx)


def test_the_state_prefix_is_one_number(lib):
    """The training layout (an image context's workspace_bytes) and the inference layout (a text context's) start behind the same
    prefix, whatever the tower, the method and the format; no context, no prefix."""
    seen = set()
    for arch_name in TINY:
        for method in METHODS:
            for weight_format in FORMATS:
                if creatable(method, weight_format):
                    rc, ctx = image_ctx(lib, arch_name, method, weight_format)
                    assert rc == 0, lib.pevit_last_error()
                    seen.add(lib.pevit_workspace_state_bytes(ctx))
                    lib.pevit_ctx_destroy(ctx)
    for tower in TEXT_TOWERS:
        rc, ctx = text_ctx(lib, tower, "bf16")
        assert rc == 0, lib.pevit_last_error()
        seen.add(lib.pevit_workspace_state_bytes(ctx))
        lib.pevit_ctx_destroy(ctx)
    assert seen == {flag_region_of_the_sources()}
    assert lib.pevit_workspace_state_bytes(None) == 0
