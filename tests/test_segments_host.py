"""Segmented predict without a GPU: the C entries of include/pevit_segments.h, what ``pevit_infer_create_slots`` refuses, the sizes
it adds, and the pure parts of ``InferenceEngine.predict_segments`` / ``predict_mixed`` (pevit_amd/serving.py) on CPU tensors with
the engine call replaced by a stub that answers every request with rows that name it."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT

from pevit_amd import _lib, serving
from pevit_amd.synth import ARCHS

from test_serving_host import create, dims_of

ENTRIES = {"pevit_infer_create_slots": 3, "pevit_load_adapter_slot": 5, "pevit_predict_segments": 6, "pevit_predict_segments_u8": 6}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def create_slots(lib, dims, slots):
    ctx = C.c_void_p()
    return lib.pevit_infer_create_slots(C.byref(dims), slots, C.byref(ctx)), ctx


# ---- the C entries --------------------------------------------------------------------------------------------------------------
def test_the_entries_are_exported_declared_and_typed(lib):
    main = open(os.path.join(ROOT, "include", "pevit_hip.h")).read()
    assert '#include "pevit_segments.h"' in main           # one include gives a C caller the whole ABI
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pevit_segments.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(pevit_[a-z0-9_]+)\s*\(", header))) == sorted(ENTRIES) == sorted(_lib.SEGMENT_SIGNATURES)
    for name, nargs in ENTRIES.items():
        res, argtypes = _lib.SEGMENT_SIGNATURES[name]
        assert res is C.c_int and len(argtypes) == nargs, name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is C.c_int
    for name in ("pevit_op_delta_add_seg", "pevit_op_attn_fwd_delta_seg"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    # the two structs as the header lays them out (LP64: three int32, padding, pointers)
    assert C.sizeof(_lib.PevitSegment) == 48 and _lib.PevitSegment.running_mean.offset == 16 and _lib.PevitSegment.features.offset == 40
    assert C.sizeof(_lib.PevitOpSegment) == 32 and _lib.PevitOpSegment.q16.offset == 16
    assert int(re.search(r"#define PEVIT_MAX_SLOTS (\d+)", header).group(1)) == _lib.MAX_SLOTS
    assert int(re.search(r"#define PEVIT_MAX_SEGMENTS_PER_CALL (\d+)", header).group(1)) == _lib.MAX_SEGMENTS


def test_create_slots_refuses_by_name_what_segments_were_not_built_for(lib):
    a = ARCHS["tiny-128"]
    ctx = C.c_void_p()
    assert lib.pevit_infer_create_slots(None, 2, C.byref(ctx)) != 0 and b"null argument" in lib.pevit_last_error()
    for slots in (0, -1, 9):
        rc, _ = create_slots(lib, dims_of(a, "kadaptation", "bf16"), slots)
        assert rc != 0 and b"slots outside [1,8]" in lib.pevit_last_error(), slots
    for method, word in (("adapter", b"Adapter"), ("compacter", b"Compacter"), ("none", b"none")):
        rc, _ = create_slots(lib, dims_of(a, method, "bf16"), 2)
        assert rc != 0 and word in lib.pevit_last_error(), method
    for method in ("kadaptation", "lora"):
        for fmt, word in (("fp8", b"fp8"), ("fp8-act", b"fp8"), ("f32-verify", b"f32 verification")):
            rc, _ = create_slots(lib, dims_of(a, method, fmt), 4)
            assert rc != 0 and word in lib.pevit_last_error(), (method, fmt)
    # bad dims are refused in the words of pevit_infer_create
    bad = _lib.PevitDims(100, 12, 32, 224, 512, 0, 4, 100)
    rc, _ = create(lib, "pevit_infer_create", bad)
    want = lib.pevit_last_error().split(b": ", 1)[1]
    rc2, _ = create_slots(lib, bad, 4)
    assert rc != 0 and rc2 != 0 and lib.pevit_last_error() == b"infer_create_slots: " + want


def test_the_sizes_a_slot_adds(lib):
    """pevit_infer_create is what it was; per slot a multi-slot context adds, per layer, 64 rows of in_proj (up to the 128-row
    padding of that matrix) and one Q panel, and 64 f32 columns of t per token."""
    for arch_name in ("tiny-128", "tiny-256", "ViT-B/32"):
        a = ARCHS[arch_name]
        E, L, N = a.width, a.layers, a.tokens
        for method in ("kadaptation", "lora"):
            d = dims_of(a, method, "bf16")
            _, plain = create(lib, "pevit_infer_create", d)
            a0, w0 = lib.pevit_arena_bytes(plain), {B: lib.pevit_workspace_bytes(plain, B) for B in (1, 5, 128)}
            for slots in (1, 2, 8):
                rc, ctx = create_slots(lib, d, slots)
                assert rc == 0, lib.pevit_last_error()
                rows = -(-(3 * E + 64 * (slots + 1)) // 128) * 128 - -(-(3 * E + 64) // 128) * 128
                extra = lib.pevit_arena_bytes(ctx) - a0
                assert L * (rows * E * 2 + slots * E * 64 * 2) <= extra <= L * (rows * E * 2 + slots * E * 64 * 2 + 2 * 256), (arch_name, slots)
                for B, w in w0.items():
                    grow = lib.pevit_workspace_bytes(ctx, B) - w
                    assert B * N * 64 * 4 * slots <= grow <= B * N * 64 * 4 * slots + 256, (arch_name, slots, B)
                lib.pevit_ctx_destroy(ctx)
            lib.pevit_ctx_destroy(plain)


def test_host_refusals_need_no_gpu(lib):
    a = ARCHS["tiny-128"]
    fake = C.c_void_p(256)
    _, plain = create(lib, "pevit_infer_create", dims_of(a, "lora", "bf16"))
    rc, multi = create_slots(lib, dims_of(a, "lora", "bf16"), 4)
    assert rc == 0
    segs = (_lib.PevitSegment * 1)()
    assert lib.pevit_load_adapter_slot(plain, None, 0, fake, 3) != 0 and b"no adapter slots" in lib.pevit_last_error()
    assert lib.pevit_load_adapter_slot(multi, None, 0, fake, 3) != 0 and b"not bound" in lib.pevit_last_error()
    assert lib.pevit_load_adapter_slot(None, None, 0, fake, 3) != 0
    assert lib.pevit_predict_segments(multi, None, fake, 1, 1, segs) != 0 and b"not bound" in lib.pevit_last_error()
    # one slot on dims that segments were not built for: the context of pevit_infer_create, which refuses the segmented calls
    rc, one = create_slots(lib, dims_of(a, "adapter", "bf16"), 1)
    _, same = create(lib, "pevit_infer_create", dims_of(a, "adapter", "bf16"))
    assert rc == 0 and lib.pevit_arena_bytes(one) == lib.pevit_arena_bytes(same)
    assert lib.pevit_workspace_bytes(one, 5) == lib.pevit_workspace_bytes(same, 5)
    for ctx in (plain, multi, one, same):
        lib.pevit_ctx_destroy(ctx)


# ---- the pure parts -------------------------------------------------------------------------------------------------------------
def test_grouping_is_stable():
    names = ["b", "a", "b", "c", "a", "b"]
    order, groups = serving.group_rows(names)
    assert order == [0, 2, 5, 1, 4, 3] and groups == [("b", 3), ("a", 2), ("c", 1)]
    assert serving.group_rows(["x"]) == ([0], [("x", 1)])
    assert [names[i] for i in order] == ["b"] * 3 + ["a"] * 2 + ["c"]


def test_scatter_back_restores_the_order_and_pads_with_minus_infinity():
    names = ["b", "a", "b", "c", "a", "b"]
    classes = {"a": 2, "b": 4, "c": 3}
    order, groups = serving.group_rows(names)
    # the answer for row i of the input names i in column 0 and its class count in the last column it owns
    outs, lo = [], 0
    for name, count in groups:
        o = torch.zeros(count, classes[name])
        o[:, 0] = torch.tensor([float(i) for i in order[lo:lo + count]])
        o[:, -1] += 100.0 * classes[name]
        outs.append(o)
        lo += count
    full = serving.scatter_rows(order, groups, outs)
    assert full.shape == (6, 4)
    for i, n in enumerate(names):
        c = classes[n]
        assert float(full[i, 0]) == i + (100.0 * c if c == 1 else 0.0) and float(full[i, c - 1]) >= 100.0 * c
        assert bool(torch.isinf(full[i, c:]).all()) and bool((full[i, c:] < 0).all()) and bool(torch.isfinite(full[i, :c]).all())


def test_chunking_never_splits_a_request():
    assert serving.chunk_requests([3, 1, 4], 8) == [[0, 1, 2]]
    assert serving.chunk_requests([3, 1, 4, 1], 8) == [[0, 1, 2], [3]]
    assert serving.chunk_requests([5, 5, 5], 8) == [[0], [1], [2]]
    assert serving.chunk_requests([8, 1, 7, 2], 8) == [[0], [1, 2], [3]]
    assert serving.chunk_requests([1] * 20, 64) == [list(range(16)), [16, 17, 18, 19]]          # 16 segments per engine call
    with pytest.raises(_lib.PevitError, match="exceeds max_batch"):
        serving.chunk_requests([3, 9], 8)
    with pytest.raises(_lib.PevitError, match="empty"):
        serving.chunk_requests([3, 0], 8)


def test_the_slot_map_loads_on_a_miss_only_and_evicts_the_least_recently_used():
    names, used, clock = [None] * 3, [0] * 3, 0
    slot_of, loads, clock = serving.assign_slots(names, used, clock, ["a", "b"])
    assert slot_of == {"a": 0, "b": 1} and loads == [(0, "a"), (1, "b")] and names == ["a", "b", None]
    slot_of, loads, clock = serving.assign_slots(names, used, clock, ["b", "a"])
    assert slot_of == {"a": 0, "b": 1} and loads == []                          # resident: nothing is loaded
    slot_of, loads, clock = serving.assign_slots(names, used, clock, ["c", "a"])
    assert slot_of == {"c": 2, "a": 0} and loads == [(2, "c")]                  # an empty slot before any eviction
    slot_of, loads, clock = serving.assign_slots(names, used, clock, ["d"])
    assert loads == [(1, "d")] and names == ["a", "d", "c"]                     # b was used longest ago
    slot_of, loads, clock = serving.assign_slots(names, used, clock, ["b", "c"])
    assert loads == [(0, "b")] and names == ["b", "d", "c"]                     # a is the oldest that this call does not want
    slot_of, loads, clock = serving.assign_slots(names, used, clock, ["a", "b", "c"])
    assert loads == [(1, "a")] and slot_of == {"a": 1, "b": 0, "c": 2}
    with pytest.raises(_lib.PevitError, match="4 adapters in one call on a context of 3 slots"):
        serving.assign_slots(names, used, clock, ["a", "b", "c", "d"])
    assert names == ["b", "a", "c"]                                             # a refused call changes nothing


class _Stub(serving.InferenceEngine):
    """The host logic of the two methods on CPU tensors: the context, the loads and the engine call are stand-ins that record."""

    def __init__(self, slots, max_batch, classes):      # (no context is created: nothing of the base __init__ runs)
        self.slots, self.max_batch, self.device = slots, max_batch, torch.device("cpu")
        self.arch = ARCHS["tiny-128"]
        self._adapters = {n: {"num_classes": c, "tag": 1000.0 * (k + 1)} for k, (n, c) in enumerate(classes.items())}
        self._slot_names, self._slot_used, self._slot_clock = [None] * slots, [0] * slots, 0
        self._input_norm, self._input_resize = None, False
        self.loaded, self.calls, self.fail_load = [], [], None

    def _load_slot(self, slot, name):
        if name == self.fail_load:
            raise _lib.PevitError("pevit_load_adapter_slot failed")
        self.loaded.append((slot, name))

    def _segments_call(self, img, parts):
        self.calls.append([(slot, count) for slot, _, count, _, _ in parts])
        assert len(img) == sum(p[2] for p in parts) <= self.max_batch
        first = 0
        for slot, a, count, logits, feat in parts:
            assert self._slot_names[slot] is not None and self._adapters[self._slot_names[slot]] is a
            logits[:] = a["tag"] + img[first:first + count, 0, 0, 0].unsqueeze(1)       # adapter tag + the row's own mark
            first += count


def marked(n, lo=0):
    img = torch.zeros(n, 3, 48, 48)
    img[:, 0, 0, 0] = torch.arange(lo, lo + n, dtype=torch.float32)
    return img


def test_predict_segments_on_a_stub():
    e = _Stub(slots=2, max_batch=8, classes={"a": 3, "b": 5, "c": 2})
    out = e.predict_segments([("a", marked(3)), ("b", marked(1, 10)), ("a", marked(4, 20))])
    assert [tuple(o.shape) for o in out] == [(3, 3), (1, 5), (4, 3)]
    assert out[0][:, 0].tolist() == [1000.0, 1001.0, 1002.0] and out[1][0, 4] == 2010.0 and out[2][:, 2].tolist() == [1020.0, 1021.0, 1022.0, 1023.0]
    assert e.calls == [[(0, 3), (1, 1), (0, 4)]] and e.loaded == [(0, "a"), (1, "b")]
    e.predict_segments([("b", marked(2)), ("a", marked(2))])
    assert e.loaded == [(0, "a"), (1, "b")]                                     # both resident: no load
    # nine images of two names on max_batch 8: two engine calls, the second request whole in the second
    e.predict_segments([("a", marked(5)), ("b", marked(4))])
    assert e.calls[-2:] == [[(0, 5)], [(1, 4)]]
    e.predict_segments([("c", marked(1)), ("b", marked(1))])
    assert e.loaded[-1] == (0, "c")                                             # a was used longest ago
    with pytest.raises(_lib.PevitError, match="3 adapters in one call on a context of 2 slots"):
        e.predict_segments([("a", marked(1)), ("b", marked(1)), ("c", marked(1))])
    with pytest.raises(_lib.PevitError, match="exceeds max_batch"):
        e.predict_segments([("a", marked(9))])
    with pytest.raises(KeyError):
        e.predict_segments([("z", marked(1))])
    with pytest.raises(_lib.PevitError, match="slots"):
        _Stub(slots=1, max_batch=8, classes={"a": 3}).predict_segments([("a", marked(1))])


def test_a_failed_load_leaves_no_name_in_a_slot_that_does_not_hold_it():
    e = _Stub(slots=3, max_batch=8, classes={"a": 3, "b": 5, "c": 2})
    e.predict_segments([("a", marked(1))])
    e.fail_load = "b"
    with pytest.raises(_lib.PevitError, match="pevit_load_adapter_slot failed"):
        e.predict_segments([("a", marked(1)), ("b", marked(1)), ("c", marked(1))])
    assert e._slot_names == ["a", None, None] and e.calls == [[(0, 1)]]          # neither the failed load nor the one behind it
    e.fail_load = None
    e.predict_segments([("b", marked(1)), ("c", marked(1))])
    assert e._slot_names == ["a", "b", "c"] and e.loaded[-2:] == [(1, "b"), (2, "c")]


def test_requests_the_segmented_call_does_not_take_are_refused_by_name():
    from pevit_amd.preprocess import RaggedBatch
    e = _Stub(slots=2, max_batch=8, classes={"a": 3, "b": 5})
    with pytest.raises(_lib.PevitError, match="uint8 and float requests in one call"):
        e.predict_segments([("a", marked(1)), ("b", marked(1).to(torch.uint8))])
    ragged = object.__new__(RaggedBatch)
    with pytest.raises(_lib.PevitError, match="ragged batch"):
        e.predict_segments([("a", ragged)])
    with pytest.raises(_lib.PevitError, match="ragged batch"):
        e.predict_mixed(ragged, ["a"])
    assert e.calls == [] and e.loaded == []


def test_predict_mixed_on_a_stub():
    e = _Stub(slots=3, max_batch=8, classes={"a": 3, "b": 5, "c": 2})
    names = ["b", "a", "b", "c", "a", "b"]
    full = e.predict_mixed(marked(6), names)
    assert full.shape == (6, 5) and e.calls == [[(0, 3), (1, 2), (2, 1)]]
    tag = {"a": 1000.0, "b": 2000.0, "c": 3000.0}
    for i, n in enumerate(names):
        c = e._adapters[n]["num_classes"]
        assert full[i, :c].tolist() == [tag[n] + i] * c                        # every row got its own adapter and came back in place
        assert bool((full[i, c:] == float("-inf")).all())
    with pytest.raises(_lib.PevitError, match="names for"):
        e.predict_mixed(marked(3), ["a", "b"])
    assert "ONE BATCH" in serving.InferenceEngine.predict_mixed.__doc__.upper()


def test_a_dropped_or_replaced_adapter_leaves_its_slot():
    e = _Stub(slots=2, max_batch=8, classes={"a": 3, "b": 5})
    e.predict_segments([("a", marked(1)), ("b", marked(1))])
    assert e._slot_names == ["a", "b"]
    e._adapters.pop("a")                          # (what drop does after _forget_slot; no stream to wait for here)
    e._forget_slot("a")
    assert e._slot_names == [None, "b"]
    e._adapters["a"] = {"num_classes": 4, "tag": 7000.0}
    out = e.predict_segments([("a", marked(2))])
    assert e.loaded[-1] == (0, "a") and out[0].shape == (2, 4) and float(out[0][1, 0]) == 7001.0
