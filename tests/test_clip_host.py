"""Gradient-norm clipping without a GPU: the three C entries of include/pevit_clip.h, every refusal of theirs (none reads a pointer or
launches), the scratch size, the config key, and where the probe's ``train_one`` puts the clip on each of its three routes -- shown
on an engine that only records its calls."""
import ctypes as C
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch
from torch import nn

from conftest import ROOT

from pevit_amd import _lib
from pevit_amd.config import default_config
from pevit_amd.synth import ARCHS

from test_serving_host import create, dims_of

ENTRIES = {"pevit_clip_scratch_floats": (C.c_size_t, 1), "pevit_clip_grad_norm": (C.c_int, 5), "pevit_op_clip_grad_norm": (C.c_int, 7)}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# ---- the C entries --------------------------------------------------------------------------------------------------------------
def test_the_entries_are_exported_declared_and_typed(lib):
    main = open(os.path.join(ROOT, "include", "pevit_hip.h")).read()
    assert '#include "pevit_clip.h"' in main               # one include gives a C caller the whole ABI
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pevit_clip.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(pevit_[a-z0-9_]+)\s*\(", header))) == sorted(ENTRIES) == sorted(_lib.CLIP_SIGNATURES)
    ctype = {"size_t": C.c_size_t, "float": C.c_float, "int": C.c_int}
    for name, (res, nargs) in ENTRIES.items():
        got_res, argtypes = _lib.CLIP_SIGNATURES[name]
        assert got_res is res and len(argtypes) == nargs, name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is res
        # the prototype of the header, argument by argument: pointers travel as void pointers
        ret, args = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)" % name, header).groups()
        assert ctype[ret] is res
        want = [C.c_void_p if "*" in a else ctype[a.split()[-2]] for a in args.split(",")]
        assert want == argtypes, name


def test_scratch_size_is_monotone_and_holds_the_three_state_words(lib):
    sizes = [lib.pevit_clip_scratch_floats(n) for n in (0, 1, 3, 64, 8191, 8192, 8193, 10**5, 2**20 + 3, 5 * 10**6, 2**33)]
    assert all(s >= 3 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]


def training_ctx(lib, method="kadaptation", with_params=True):
    rc, ctx = create(lib, "pevit_ctx_create", dims_of(ARCHS["tiny-128"], method, "bf16"))
    assert rc == 0, lib.pevit_last_error()
    fake = C.c_void_p(256)
    if with_params:
        assert lib.pevit_set_params(ctx, fake, fake, fake, fake) == 0
    return ctx


def test_every_refusal_comes_with_its_words_and_without_a_device(lib):
    fake = C.c_void_p(256)                                  # never read: a refusal launches nothing
    ctx = training_ctx(lib)
    assert lib.pevit_clip_grad_norm(None, None, 1.0, 1.0, fake) != 0 and b"null context" in lib.pevit_last_error()
    assert lib.pevit_clip_grad_norm(ctx, None, 1.0, 1.0, None) != 0 and b"null scratch" in lib.pevit_last_error()
    for bad in (0.0, -1.0, math.nan, math.inf):
        assert lib.pevit_clip_grad_norm(ctx, None, bad, 1.0, fake) != 0, bad
        assert b"max_norm" in lib.pevit_last_error() and b"finite and positive" in lib.pevit_last_error(), bad
        assert lib.pevit_op_clip_grad_norm(None, fake, None, 100, bad, 1.0, fake) != 0, bad
        assert b"max_norm" in lib.pevit_last_error(), bad
    for bad in (0.0, -0.5, math.nan, math.inf):
        assert lib.pevit_clip_grad_norm(ctx, None, 1.0, bad, fake) != 0, bad
        assert b"grad_scale" in lib.pevit_last_error() and b"finite and positive" in lib.pevit_last_error(), bad
        assert lib.pevit_op_clip_grad_norm(None, fake, None, 100, 1.0, bad, fake) != 0 and b"grad_scale" in lib.pevit_last_error(), bad
    lib.pevit_ctx_destroy(ctx)
    # a context without parameters (no gradient buffer)
    bare = training_ctx(lib, with_params=False)
    assert lib.pevit_clip_grad_norm(bare, None, 1.0, 1.0, fake) != 0 and b"parameters not set" in lib.pevit_last_error()
    lib.pevit_ctx_destroy(bare)
    # an inference-only and a text context
    rc, infer = create(lib, "pevit_infer_create", dims_of(ARCHS["tiny-128"], "kadaptation", "bf16"))
    assert rc == 0
    assert lib.pevit_clip_grad_norm(infer, None, 1.0, 1.0, fake) != 0 and b"inference-only context" in lib.pevit_last_error()
    lib.pevit_ctx_destroy(infer)
    text = C.c_void_p()
    assert lib.pevit_text_create(C.byref(_lib.PevitTextDims(128, 2, 8, 64, 64, 0)), C.byref(text)) == 0, lib.pevit_last_error()
    assert lib.pevit_clip_grad_norm(text, None, 1.0, 1.0, fake) != 0 and b"text context" in lib.pevit_last_error()
    lib.pevit_ctx_destroy(text)
    # the context-free entry: null pointers, an empty buffer, pointers the 16-byte loads cannot take
    assert lib.pevit_op_clip_grad_norm(None, None, None, 100, 1.0, 1.0, fake) != 0 and b"null argument" in lib.pevit_last_error()
    assert lib.pevit_op_clip_grad_norm(None, fake, None, 100, 1.0, 1.0, None) != 0 and b"null argument" in lib.pevit_last_error()
    assert lib.pevit_op_clip_grad_norm(None, fake, None, 0, 1.0, 1.0, fake) != 0 and b"empty buffer" in lib.pevit_last_error()
    assert lib.pevit_op_clip_grad_norm(None, C.c_void_p(260), None, 100, 1.0, 1.0, fake) != 0 and b"16-byte aligned" in lib.pevit_last_error()
    assert lib.pevit_op_clip_grad_norm(None, fake, C.c_void_p(257), 100, 1.0, 1.0, fake) != 0 and b"4-byte aligned" in lib.pevit_last_error()


def test_the_key_exists_and_is_off():
    cfg = default_config()
    assert cfg.TRAIN.CLIP_GRAD_NORM == 0.0
    cfg.merge_from_list(["TRAIN.CLIP_GRAD_NORM", "1.5"])
    assert cfg.TRAIN.CLIP_GRAD_NORM == 1.5


def test_the_host_surface_takes_the_bound_and_defaults_to_off():
    import inspect
    from pevit_amd.engine import HipEngine
    from pevit_amd.evaluation._harness import ClassifierBase
    from pevit_amd import engine_optim
    assert inspect.signature(ClassifierBase.fused_train_step).parameters["max_grad_norm"].default is None
    assert list(inspect.signature(engine_optim.clip_grad_norm).parameters) == ["engine", "max_norm", "grad_scale"]
    assert inspect.signature(engine_optim.clip_grad_norm).parameters["grad_scale"].default == 1.0
    # the bound of the steps is an attribute of the engine, declared (off) in __init__ with the rest of its state; every update
    # goes through _update, which reads it
    init = inspect.getsource(HipEngine.__init__)
    assert "self.max_grad_norm = None" in init and "self.last_grad_norm = self._clip_scratch[0]" in init
    assert "self.max_grad_norm" in inspect.getsource(HipEngine._update)
    assert "self.max_grad_norm" in inspect.getsource(HipEngine.capture_train_step)
    seen = []
    eng = SimpleNamespace(_clip_grad_norm=lambda m, s: seen.append((m, s)) or "norm")
    assert engine_optim.clip_grad_norm(eng, 2.0) == "norm" and seen == [(2.0, 1.0)]


# ---- where the clip sits in the probe's train_one: an engine that records its calls ------------------------------------------------
D, CLASSES, ROWS, BATCH = 16, 5, 24, 8


class RecordingEngine:
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def ensure_batch(self, n):
        pass

    def probe_step(self, feats, index, labels, **kw):
        self.calls.append(("probe_step", {k: v for k, v in kw.items() if k not in ("logits_out", "loss_out")}))
        kw["logits_out"].zero_(); kw["loss_out"].zero_()

    def _clip_grad_norm(self, max_norm, grad_scale=1.0):      # what engine_optim.clip_grad_norm(engine, ...) calls
        self.calls.append(("clip_grad_norm", (max_norm, grad_scale)))

    def sgd_step(self, **kw):
        self.calls.append(("sgd_step", kw))

    def optimizer_step(self, plan):
        self.calls.append(("optimizer_step", plan))


class Loader:
    """What train_one reads of a TensorLoader: its length, its dataset's length and the epoch's index batches."""
    dataset = range(ROWS)

    def __len__(self):
        return ROWS // BATCH

    def iter_indices(self):
        return iter(torch.arange(ROWS).split(BATCH))


class Plan:
    def refresh(self, optimizer):
        return self


class Model(nn.Module):
    def __init__(self, route):
        super().__init__()
        self.layers = nn.Sequential(nn.Linear(D, CLASSES))
        self.channel_bn = nn.BatchNorm1d(D, affine=False)
        self.route, self.eng, self.the_plan = route, RecordingEngine(), Plan()
        g = torch.Generator().manual_seed(0)
        self.cache = SimpleNamespace(feats=torch.randn(ROWS, D, generator=g), labels=torch.randint(0, CLASSES, (ROWS,), generator=g))

    def cached(self, loader):
        return self.cache

    def probe_route(self, criterion, optimizer, cache):
        return self.route, (self.the_plan if self.route == "plan" else None)

    def engine(self):
        return self.eng

    def scale(self):
        return 1.0

    def head(self, feature):
        return self.layers(self.channel_bn(feature))

    def flush_bn_counter(self, *_):
        pass


def run_epoch(route, clip):
    from pevit_amd.evaluation import full_model_finetune as fmf
    cfg = default_config()
    assert cfg.TRAIN.CLIP_GRAD_NORM == 0.0                  # the key exists; off unless a run sets it
    cfg.DATASET.NUM_CLASSES = CLASSES
    cfg.TRAIN.CLIP_GRAD_NORM = clip
    model = Model(route)
    opt = torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True)
    fmf.train_one(Loader(), model, nn.CrossEntropyLoss(), opt, 0, cfg)
    return model


HYPER = dict(lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True)


def step_kwargs(update):
    return dict(HYPER, bn_training=True, scale=1.0, update=update)


def test_fused_route_with_the_key_takes_the_step_apart():
    m = run_epoch("fused", 1.0)
    one = [("probe_step", step_kwargs(False)), ("clip_grad_norm", (1.0, 1.0)), ("sgd_step", HYPER)]
    assert m.eng.calls == one * (ROWS // BATCH)


def test_plan_route_with_the_key_clips_between_the_gradients_and_the_planned_update():
    m = run_epoch("plan", 1.0)
    one = [("probe_step", step_kwargs(False)), ("clip_grad_norm", (1.0, 1.0)), ("optimizer_step", m.the_plan)]
    assert m.eng.calls == one * (ROWS // BATCH)


@pytest.mark.parametrize("key", [0.0, -1.0])
def test_without_the_key_the_calls_are_those_of_before(key):
    m = run_epoch("fused", key)
    assert m.eng.calls == [("probe_step", step_kwargs(True))] * (ROWS // BATCH)
    m = run_epoch("plan", key)
    assert m.eng.calls == [("probe_step", step_kwargs(False)), ("optimizer_step", m.the_plan)] * (ROWS // BATCH)


def test_autograd_route_calls_torch_clip_once_per_step(monkeypatch):
    seen, real = [], torch.nn.utils.clip_grad_norm_

    def spy(parameters, max_norm, *a, **kw):
        seen.append(max_norm)
        return real(parameters, max_norm, *a, **kw)
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", spy)
    m = run_epoch("autograd", 0.25)
    assert seen == [0.25] * (ROWS // BATCH) and m.eng.calls == []
    seen.clear()
    run_epoch("autograd", 0.0)
    assert seen == []


def test_peft_train_one_hands_the_key_to_the_fused_step_and_to_torch_elsewhere(monkeypatch):
    """The shared harness: a fused step gets ``max_grad_norm`` (and only with the key on: the call of before otherwise); the
    route that runs torch's ``step()`` clips with torch."""
    from pevit_amd.evaluation import _harness as h

    class Peft(nn.Module):
        def __init__(self, fuse):
            super().__init__()
            self.lin, self.fuse, self.steps = nn.Linear(D, CLASSES), fuse, []

        def can_fuse(self, criterion, optimizer):
            return self.fuse

        def fused_optimizer_plan(self, criterion, optimizer):
            return None

        def forward(self, x):
            return self.lin(x)

        def fused_train_step(self, images, target, optimizer, logits_out=None, loss_out=None, **kw):
            self.steps.append(kw)
            return torch.zeros(images.shape[0], CLASSES), torch.zeros(1)

        def flush_bn_counter(self, *_):
            pass

    g = torch.Generator().manual_seed(1)
    batches = [(torch.randn(BATCH, D, generator=g), torch.randint(0, CLASSES, (BATCH,), generator=g)) for _ in range(2)]
    monkeypatch.setattr(h, "DeviceFeeder", lambda loader, dev: loader)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **kw: self)
    seen, real = [], torch.nn.utils.clip_grad_norm_
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", lambda p, m, *a, **kw: (seen.append(m), real(p, m, *a, **kw))[1])
    for key, want_kw, want_torch in ((0.0, {"plan": None}, []), (2.0, {"plan": None, "max_grad_norm": 2.0}, [2.0, 2.0])):
        cfg = default_config()
        assert cfg.TRAIN.CLIP_GRAD_NORM == 0.0
        cfg.DATASET.NUM_CLASSES = CLASSES
        cfg.TRAIN.CLIP_GRAD_NORM = key
        fused = Peft(True)
        h.train_one(batches, fused, nn.CrossEntropyLoss(), torch.optim.SGD(fused.parameters(), lr=0.1), 0, cfg)
        assert fused.steps == [want_kw] * 2 and seen == []
        plain = Peft(False)
        h.train_one(batches, plain, nn.CrossEntropyLoss(), torch.optim.SGD(plain.parameters(), lr=0.1), 0, cfg)
        assert plain.steps == [] and seen == want_torch
        seen.clear()
