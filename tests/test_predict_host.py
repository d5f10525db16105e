"""CPU-side checks of the inference path's boundary: the cross-compiled library exports pevit_predict / pevit_predict_u8, the header
declares them with the documented arguments, the ctypes table carries their argument types, the epilogue ids of kernels.h stay
unique (the new one included), and an unbound context refuses the call."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

from pevit_amd import _lib


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _header():
    return open(os.path.join(ROOT, "include", "pevit_hip.h")).read()


@pytest.mark.parametrize("name,pixels", [("pevit_predict", "const float*"), ("pevit_predict_u8", "const uint8_t*")])
def test_predict_entries_are_exported_declared_and_typed(lib, name, pixels):
    assert hasattr(lib, name), f"{name} is not exported by the library"
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{name} is not declared in include/pevit_hip.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert [a.rsplit(" ", 1)[0] for a in args] == ["pevit_ctx*", "void*", pixels, "const float*", "const float*", "float*",
                                                   "float*", "int"]           # the running buffers are const: only read
    res, argtypes = _lib.SIGNATURES[name]
    assert res is C.c_int and argtypes == [C.c_void_p] * 7 + [C.c_int]
    fn = getattr(lib, name)
    assert fn.restype is C.c_int and list(fn.argtypes) == argtypes


def test_epilogue_ids_are_unique_and_dense():
    src = open(os.path.join(ROOT, "pevit_amd", "csrc", "kernels.h")).read()
    body = re.search(r"enum GemmEpilogue \{(.*?)\};", src, flags=re.S).group(1)
    ids = dict(re.findall(r"^\s*(EPI_[A-Z0-9_]+)\s*=\s*(\d+)\s*,", body, flags=re.M))
    assert "EPI_BIAS_GELU" in ids and "EPI_BIAS_GELU_ONLY" in ids
    values = sorted(int(v) for v in ids.values())
    assert values == list(range(len(values))), ids                # unique, and the launch table indexes them 0 .. last
    assert int(ids["EPI_BIAS_GELU_ONLY"]) == max(values)
    assert re.search(r"constexpr int EPI_LAST = EPI_BIAS_GELU_ONLY;", src)


def test_predict_refuses_an_unbound_context(lib):
    d = _lib.PevitDims(128, 2, 16, 48, 64, 0, 4, 10)
    ctx = C.c_void_p()
    assert lib.pevit_ctx_create(C.byref(d), C.byref(ctx)) == 0
    assert lib.pevit_predict(ctx, None, None, None, None, None, None, 1) != 0
    assert b"not bound" in lib.pevit_last_error()
    assert lib.pevit_predict_u8(ctx, None, None, None, None, None, None, 1) != 0
    assert b"pevit_set_input_norm" in lib.pevit_last_error()
    lib.pevit_ctx_destroy(ctx)
