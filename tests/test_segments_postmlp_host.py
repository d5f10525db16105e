"""Segmented predict for the post-MLP methods without a GPU: the C entries of include/pevit_segments_all.h, what
``pevit_infer_create_slots_all`` creates, adds and refuses, and the host refusals of the slot loaders.  The entries of
include/pevit_segments.h stay what tests/test_segments_host.py pins them to be."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

from pevit_amd import _lib, serving
from pevit_amd.synth import ARCHS

from test_serving_host import create, dims_of

ENTRIES = {"pevit_infer_create_slots_all": 3, "pevit_load_adapter_slot_rule": 6}
POST_MLP = ("adapter", "compacter")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def create_all(lib, dims, slots):
    ctx = C.c_void_p()
    return lib.pevit_infer_create_slots_all(C.byref(dims), slots, C.byref(ctx)), ctx


def create_slots(lib, dims, slots):
    ctx = C.c_void_p()
    return lib.pevit_infer_create_slots(C.byref(dims), slots, C.byref(ctx)), ctx


def test_the_entries_are_exported_declared_and_typed(lib):
    main = open(os.path.join(ROOT, "include", "pevit_hip.h")).read()
    assert '#include "pevit_segments_all.h"' in main           # one include gives a C caller the whole ABI
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pevit_segments_all.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(pevit_[a-z0-9_]+)\s*\(", header))) == sorted(ENTRIES) == sorted(_lib.SEGMENT_ALL_SIGNATURES)
    for name, nargs in ENTRIES.items():
        res, argtypes = _lib.SEGMENT_ALL_SIGNATURES[name]
        assert res is C.c_int and len(argtypes) == nargs, name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is C.c_int
    assert "pevit_op_adapter_fwd_seg" in _lib.SIGNATURES and hasattr(lib, "pevit_op_adapter_fwd_seg")
    # the two structs of the kernel's test entry as the header lays them out (LP64)
    assert C.sizeof(_lib.PevitAdapterSeg) == 56 and _lib.PevitAdapterSeg.gamma.offset == 8 and _lib.PevitAdapterSeg.b_up.offset == 48
    assert C.sizeof(_lib.PevitAdapterFwdSegArgs) == 56 and _lib.PevitAdapterFwdSegArgs.segs.offset == 32
    assert _lib.PevitAdapterFwdSegArgs.act_kind.offset == 40
    src = re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    for struct, cls in (("pevit_adapter_seg", _lib.PevitAdapterSeg), ("pevit_adapter_fwd_seg_args", _lib.PevitAdapterFwdSegArgs)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl.startswith("int32_t"):
                names += [n.strip() for n in decl[len("int32_t"):].split(",")]
            elif decl:
                names.append(decl.split("*")[-1].strip())
        assert [n for n, _ in cls._fields_] == names, struct


@pytest.mark.parametrize("method", POST_MLP)
@pytest.mark.parametrize("arch_name", ["tiny-128", "tiny-256", "ViT-B/32"])
def test_post_mlp_slot_contexts_are_created_and_what_a_slot_adds(lib, arch_name, method):
    """The workspace is that of pevit_infer_create byte for byte; per layer and slot the arena grows by one [64][E] and one [E][64]
    bf16 panel (up to the 256-byte alignment of the two runs of panels) and by nothing else; one slot is pevit_infer_create."""
    a = ARCHS[arch_name]
    E, L = a.width, a.layers
    d = dims_of(a, method, "bf16")
    rc, plain = create(lib, "pevit_infer_create", d)
    assert rc == 0
    a0, w0 = lib.pevit_arena_bytes(plain), {B: lib.pevit_workspace_bytes(plain, B) for B in (1, 5, 128)}
    for slots in (1, 2, 8):
        rc, ctx = create_all(lib, d, slots)
        assert rc == 0, lib.pevit_last_error()
        for B, w in w0.items():
            assert lib.pevit_workspace_bytes(ctx, B) == w, (slots, B)
        extra = lib.pevit_arena_bytes(ctx) - a0
        if slots == 1:
            assert extra == 0
        else:
            panels = slots * 2 * 64 * E * 2
            assert L * panels <= extra <= L * (panels + 2 * 256), (arch_name, slots, extra)
        assert lib.pevit_num_tower_params(ctx) == lib.pevit_num_tower_params(plain)
        lib.pevit_ctx_destroy(ctx)
    lib.pevit_ctx_destroy(plain)


def test_the_site_methods_get_the_context_of_the_existing_entry(lib):
    for arch_name in ("tiny-128", "ViT-B/32"):
        a = ARCHS[arch_name]
        for method in ("kadaptation", "lora"):
            d = dims_of(a, method, "bf16")
            for slots in (1, 2, 8):
                (r1, new), (r2, old) = create_all(lib, d, slots), create_slots(lib, d, slots)
                assert r1 == 0 and r2 == 0
                assert lib.pevit_arena_bytes(new) == lib.pevit_arena_bytes(old)
                for B in (1, 5, 128):
                    assert lib.pevit_workspace_bytes(new, B) == lib.pevit_workspace_bytes(old, B)
                lib.pevit_ctx_destroy(new)
                lib.pevit_ctx_destroy(old)
            # ... and its refusals, in its words
            for fmt in ("fp8", "fp8-act", "f32-verify"):
                r1, _ = create_all(lib, dims_of(a, method, fmt), 4)
                m1 = lib.pevit_last_error()
                r2, _ = create_slots(lib, dims_of(a, method, fmt), 4)
                assert r1 != 0 and r2 != 0 and m1 == lib.pevit_last_error()


def test_create_refuses_by_name(lib):
    a = ARCHS["tiny-128"]
    ctx = C.c_void_p()
    assert lib.pevit_infer_create_slots_all(None, 2, C.byref(ctx)) != 0 and b"null argument" in lib.pevit_last_error()
    assert lib.pevit_infer_create_slots_all(C.byref(dims_of(a, "adapter", "bf16")), 2, None) != 0 and b"null argument" in lib.pevit_last_error()
    for method in POST_MLP + ("none",):
        for slots in (0, -1, 9):
            rc, _ = create_all(lib, dims_of(a, method, "bf16"), slots)
            assert rc != 0 and b"slots outside [1,8]" in lib.pevit_last_error(), (method, slots)
    rc, _ = create_all(lib, dims_of(a, "none", "bf16"), 2)
    assert rc != 0 and b"none" in lib.pevit_last_error()
    for method in POST_MLP:
        for fmt, word in (("fp8", b"fp8"), ("fp8-act", b"fp8"), ("f32-verify", b"f32 verification")):
            rc, _ = create_all(lib, dims_of(a, method, fmt), 4)
            msg = lib.pevit_last_error()
            assert rc != 0 and word in msg and msg.startswith(b"infer_create_slots_all: 4 slots"), (method, fmt, msg)
    # bad dims are refused in the words of pevit_infer_create
    bad = _lib.PevitDims(100, 12, 32, 224, 512, _lib.METHOD_IDS["adapter"], 4, 100)
    rc, _ = create(lib, "pevit_infer_create", bad)
    want = lib.pevit_last_error().split(b": ", 1)[1]
    rc2, _ = create_all(lib, bad, 4)
    assert rc != 0 and rc2 != 0 and lib.pevit_last_error() == b"infer_create_slots_all: " + want


def test_the_existing_entry_still_refuses_the_post_mlp_methods(lib):
    a = ARCHS["tiny-128"]
    for method, word in (("adapter", b"Adapter"), ("compacter", b"Compacter")):
        rc, _ = create_slots(lib, dims_of(a, method, "bf16"), 2)
        assert rc != 0 and word in lib.pevit_last_error(), method


def test_slot_loading_refusals_need_no_gpu(lib):
    a = ARCHS["tiny-128"]
    fake, rule = C.c_void_p(256), C.c_void_p(512)
    (r1, ad), (r2, co) = create_all(lib, dims_of(a, "adapter", "bf16"), 4), create_all(lib, dims_of(a, "compacter", "bf16"), 4)
    (r3, lo), (r4, one) = create_all(lib, dims_of(a, "lora", "bf16"), 4), create_all(lib, dims_of(a, "compacter", "bf16"), 1)
    assert r1 == 0 and r2 == 0 and r3 == 0 and r4 == 0
    segs = (_lib.PevitSegment * 1)()
    # unbound contexts
    assert lib.pevit_load_adapter_slot_rule(ad, None, 0, fake, 3, None) != 0 and b"not bound" in lib.pevit_last_error()
    assert lib.pevit_load_adapter_slot_rule(co, None, 0, fake, 3, rule) != 0 and b"not bound" in lib.pevit_last_error()
    assert lib.pevit_load_adapter_slot_rule(lo, None, 0, fake, 3, None) != 0 and b"not bound" in lib.pevit_last_error()
    assert lib.pevit_load_adapter_slot(ad, None, 0, fake, 3) != 0 and b"not bound" in lib.pevit_last_error()
    assert lib.pevit_predict_segments(ad, None, fake, 1, 1, segs) != 0 and b"not bound" in lib.pevit_last_error()
    # a rule where there is none to take, none where one is needed
    assert lib.pevit_load_adapter_slot_rule(ad, None, 0, fake, 3, rule) != 0 and b"only Compacter" in lib.pevit_last_error()
    assert lib.pevit_load_adapter_slot_rule(lo, None, 0, fake, 3, rule) != 0 and b"only Compacter" in lib.pevit_last_error()
    assert lib.pevit_load_adapter_slot_rule(co, None, 0, fake, 3, None) != 0 and b"phm_rule" in lib.pevit_last_error()
    assert lib.pevit_load_adapter_slot(co, None, 0, fake, 3) != 0 and b"pevit_load_adapter_slot_rule" in lib.pevit_last_error()
    # null arguments, and a context without slots
    assert lib.pevit_load_adapter_slot_rule(None, None, 0, fake, 3, None) != 0
    assert lib.pevit_load_adapter_slot_rule(ad, None, 0, None, 3, None) != 0 and b"null argument" in lib.pevit_last_error()
    assert lib.pevit_load_adapter_slot_rule(one, None, 0, fake, 3, rule) != 0 and b"no adapter slots" in lib.pevit_last_error()
    for ctx in (ad, co, lo, one):
        lib.pevit_ctx_destroy(ctx)


def test_the_docstring_says_which_rows_a_row_depends_on():
    doc = " ".join(serving.InferenceEngine.predict_mixed.__doc__.split())
    assert "depend on no other row" in doc and "ONE BATCH" in doc.upper()
