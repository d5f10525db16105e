"""CPU-side checks of the host owners (``HipEngine``, ``TextEngine``): their class surface is the recorded one, the tensor-contract
checkers accept and refuse what they always did with the same words, the generation bookkeeping of every forward entry, and no
state that appears after ``__init__``."""
import ast
import inspect
import os

import pytest
import torch

from conftest import ROOT

from pevit_amd._lib import PevitError
from pevit_amd.engine import HipEngine
from pevit_amd.synth import ARCHS
from pevit_amd.text_engine import TextEngine

KEPT_PRIVATE = ("_adam_state", "_train_step_pipelined")       # called from outside the class (bench.py, tests)

# recorded from the single-file engine; the one difference since is head_forward_backward's optional ``out`` triple
HIP_ENGINE_SURFACE = [
    "PROF_KINDS = {0: 'ln_fwd', 1: 'ln_bwd', 2: 'attn_fwd', 3: 'attn_bwd', 4: 'delta_add', 5: 'lowrank_u', 6: 'lowrank_grad', "
    "7: 'im2col', 8: 'lowrank_bwd', 9: 'attn_fwd_delta', 10: 'adapter_fwd', 11: 'adapter_bwd'}",
    "STREAMK_CHECK_EVERY = 64",
    "_adam_state(self)",
    "_train_step_pipelined(self, images, labels, lr, momentum, weight_decay, bn_training, process_group, world_size, nesterov, "
    "logits_out, loss_out, optimizer=None)",
    "attention_backward(self, dy_nbe: 'torch.Tensor', layer: 'int', need_dx: 'bool' = True)",
    "attention_forward(self, x_nbe: 'torch.Tensor', layer: 'int', save: 'bool' = True, weights: 'str | None' = None)",
    "average_bn_buffers(self, process_group=None)",
    "blocks_backward(self, dy_nbe: 'torch.Tensor', l_lo: 'int', l_hi: 'int', need_dx: 'bool' = True)",
    "blocks_forward(self, x_nbe: 'torch.Tensor', l_lo: 'int', l_hi: 'int', save: 'bool' = True) -> 'torch.Tensor'",
    "capture_train_step(self, images, labels, lr=None, momentum=0.9, weight_decay=0.0, bn_training=True, nesterov=False, "
    "optimizer=None)",
    "check_streamk(self)",
    "clear_streamk_error(self) -> 'bool'",
    "dp_exchange_mode = 'single'",
    "dp_flush(self)",
    "dp_pipeline_off(self)",
    "encode_image(self, images: 'torch.Tensor') -> 'torch.Tensor'",
    "ensure_batch(self, batch: 'int')",
    "exchange_times_us(self)",
    "forward_backward(self, images, labels, bn_training=True, logits_out=None, loss_out=None)",
    "forward_backward_dp(self, images, labels, bn_training=True, process_group=None, mode=None)",
    "grad_views(self)",
    "head_forward_backward(self, feat, labels, bn_training=True, need_dfeat=True, out=None)",
    "load_phm_rule(self, rule: 'torch.Tensor')",
    "load_state_dict(self, sd, prefix: 'str' = 'visual.')",
    "load_trainable(self, sd)",
    "optimizer_step(self, plan: \"'OptimPlan'\", grad_scale=1.0, _pipelined=False)",
    "param_views(self, buf: 'torch.Tensor | None' = None) -> \"'OrderedDict[str, torch.Tensor]'\"",
    "predict(self, images: 'torch.Tensor', logits_out=None, return_features: 'bool' = False)",
    "probe_predict(self, feats, index=None, first_row=0, count=None, scale=1.0, logits_out=None)",
    "probe_step(self, feats, index, labels, lr=0.0, momentum=0.9, weight_decay=0.0, nesterov=False, bn_training=True, scale=1.0, "
    "update=True, logits_out=None, loss_out=None)",
    "profile_gemms(self, fn, max_launches=8192, all_kernels=False)",
    "reset_optimizer(self)",
    "reset_run(self)",
    "resize_u8(self, images: 'torch.Tensor') -> 'torch.Tensor'",
    "set_input_normalization(self, mean, std)",
    "set_input_resize(self, on: 'bool' = True, center_crop: 'bool' = True)",
    "sgd_step(self, lr, momentum=0.9, weight_decay=0.0, grad_scale=1.0, nesterov=False, _pipelined=False)",
    "sync_replicas(self, process_group=None, src: 'int' = 0)",
    "time_exchange(self, on: 'bool' = True)",
    "train_step(self, images, labels, lr=None, momentum=0.9, weight_decay=0.0, bn_training=True, process_group=None, world_size=1, "
    "nesterov=False, logits_out=None, loss_out=None, optimizer=None)",
    "transformer_backward(self, dy_nbe: 'torch.Tensor', need_dx: 'bool' = True)",
    "transformer_forward(self, x_nbe: 'torch.Tensor', save: 'bool' = True) -> 'torch.Tensor'",
    "tune(self, key: 'str', value: 'int') -> 'int'",
    "use_flat_allreduce(self, process_group=None)",
    "visual_backward(self, dfeat: 'torch.Tensor')",
    "visual_forward(self, images: 'torch.Tensor', save: 'bool' = True) -> 'torch.Tensor'",
    "zero_grad(self)",
    "zeroshot(self, images: 'torch.Tensor', text_cd: 'torch.Tensor', scale: 'float' = 100.0, probs_out=None, "
    "return_logits: 'bool' = False, return_features: 'bool' = False)",
]
TEXT_ENGINE_SURFACE = ["encode(self, tokens: 'torch.Tensor') -> 'torch.Tensor'", "load_state_dict(self, sd)"]


def surface(cls):
    """Public methods (with their signatures) and class attributes (with their values), plus the private names others call."""
    out = []
    for name in sorted(n for n in dir(cls) if not n.startswith("_") or n in KEPT_PRIVATE):
        v = inspect.getattr_static(cls, name)
        out.append(f"{name}{inspect.signature(v)}" if callable(v) else f"{name} = {v!r}")
    return out


@pytest.mark.parametrize("cls, want", [(HipEngine, HIP_ENGINE_SURFACE), (TextEngine, TEXT_ENGINE_SURFACE)])
def test_surface_is_the_recorded_one(cls, want):
    assert surface(cls) == want


# ---------------------------------------------------------------------------------------------------------- the contract checkers
@pytest.fixture
def bare():
    """A HipEngine without a context: what the checkers and the generation bookkeeping read, and nothing else."""
    eng = object.__new__(HipEngine)
    eng.device, eng.arch, eng.num_classes, eng.max_batch = torch.device("cpu"), ARCHS["tiny-128"], 5, 4
    eng._input_norm = eng._pipe = None
    eng.forward_generation, eng.block_generation, eng.attention_generation = 0, {}, {}
    return eng


def refused(fn, *args):
    with pytest.raises(PevitError) as e:
        fn(*args)
    return str(e.value)


IMAGES = "images must be a contiguous float32 tensor (B,3,48,48) on cpu (or uint8 after set_input_normalization); got "
BAD_IMAGES = [
    (lambda: torch.zeros(2, 3, 48, 48, dtype=torch.float64), "(2, 3, 48, 48) torch.float64 on cpu"),
    (lambda: torch.zeros(2, 3, 32, 48), "(2, 3, 32, 48) torch.float32 on cpu"),
    (lambda: torch.zeros(2, 48, 48, 3).permute(0, 3, 1, 2), "(2, 3, 48, 48) torch.float32 on cpu"),
    (lambda: torch.zeros(2, 3, 48, 48, device="meta"), "(2, 3, 48, 48) torch.float32 on meta"),
    (lambda: torch.zeros(2, 3, 48, 48, dtype=torch.uint8), "(2, 3, 48, 48) torch.uint8 on cpu"),      # before the constants
]


def test_check_batch(bare):
    good = torch.zeros(2, 3, 48, 48)
    assert bare._check_batch(good) is None
    assert bare._check_batch(good, torch.zeros(2, dtype=torch.int64)) is False
    assert bare._check_batch(good, torch.zeros(2, 5)) is True
    for make, got in BAD_IMAGES:
        assert refused(bare._check_batch, make()) == IMAGES + got
    assert refused(bare._check_batch, torch.zeros(5, 3, 48, 48)) == "batch 5 exceeds the bound workspace (4): call ensure_batch"
    bare._input_norm = ((0.5, 0.5, 0.5), (0.25, 0.25, 0.25))
    assert bare._check_batch(torch.zeros(4, 3, 48, 48, dtype=torch.uint8)) is None
    assert refused(bare._check_batch, torch.zeros(2, 3, 32, 48, dtype=torch.uint8)) == IMAGES + "(2, 3, 32, 48) torch.uint8 on cpu"
    assert refused(bare._check_batch, good, torch.zeros(3, dtype=torch.int64)).startswith("labels must be")


def test_check_labels(bare):
    assert bare._check_labels(torch.zeros(3, dtype=torch.int64), 3) is False
    assert bare._check_labels(torch.zeros(3, 5), 3) is True
    head = "labels must be a contiguous int64 tensor (3,) or float32 tensor (3, 5) on cpu; got "
    for bad, got in [(torch.zeros(3, dtype=torch.int32), "(3,) torch.int32 on cpu"),
                     (torch.zeros(4, dtype=torch.int64), "(4,) torch.int64 on cpu"),
                     (torch.zeros(3, 4), "(3, 4) torch.float32 on cpu"),
                     (torch.zeros(3, 5, dtype=torch.int64), "(3, 5) torch.int64 on cpu"),
                     (torch.zeros(5, 3).t(), "(3, 5) torch.float32 on cpu"),
                     (torch.zeros(6, dtype=torch.int64)[::2], "(3,) torch.int64 on cpu"),
                     (torch.zeros(3, dtype=torch.int64, device="meta"), "(3,) torch.int64 on meta")]:
        assert refused(bare._check_labels, bad, 3) == head + got


def test_check_cache(bare):
    feats = torch.zeros(6, 64)
    assert bare._check_cache(feats) is None
    assert bare._check_cache(feats, torch.zeros(3, dtype=torch.int64)) is None
    assert bare._check_cache(feats, None, torch.zeros(6, dtype=torch.int64)) is False
    assert bare._check_cache(feats, torch.zeros(3, dtype=torch.int64), torch.zeros(6, 5)) is True
    head = "cached features must be a contiguous float32 tensor (rows, 64) on cpu; got "
    for bad, got in [(torch.zeros(6, 64, dtype=torch.float64), "(6, 64) torch.float64 on cpu"),
                     (torch.zeros(6, 32), "(6, 32) torch.float32 on cpu"),
                     (torch.zeros(64), "(64,) torch.float32 on cpu"),
                     (torch.zeros(0, 64), "(0, 64) torch.float32 on cpu"),
                     (torch.zeros(64, 6).t(), "(6, 64) torch.float32 on cpu"),
                     (torch.zeros(6, 64, device="meta"), "(6, 64) torch.float32 on meta")]:
        assert refused(bare._check_cache, bad) == head + got
    head = "index must be a contiguous int64 vector on cpu; got "
    for bad, got in [(torch.zeros(3, dtype=torch.int32), "(3,) torch.int32 on cpu"),
                     (torch.zeros(3, 1, dtype=torch.int64), "(3, 1) torch.int64 on cpu"),
                     (torch.zeros(6, dtype=torch.int64)[::2], "(3,) torch.int64 on cpu"),
                     (torch.zeros(3, dtype=torch.int64, device="meta"), "(3,) torch.int64 on meta")]:
        assert refused(bare._check_cache, feats, bad) == head + got
    assert refused(bare._check_cache, feats, None, torch.zeros(5, dtype=torch.int64)) == \
        "labels must be a contiguous int64 tensor (6,) or float32 tensor (6, 5) on cpu; got (5,) torch.int64 on cpu"


def test_out_buf(bare):
    good = torch.zeros(2, 5)
    assert bare._out_buf(good, (2, 5)) is good
    assert bare._out_buf(good, [2, 5]) is good
    head = "output buffer must be a contiguous float32 tensor (2, 5) on cpu; got "
    for bad, got in [(torch.zeros(2, 5, dtype=torch.float16), "(2, 5) torch.float16 on cpu"),
                     (torch.zeros(3, 5), "(3, 5) torch.float32 on cpu"),
                     (torch.zeros(10), "(10,) torch.float32 on cpu"),
                     (torch.zeros(5, 2).t(), "(2, 5) torch.float32 on cpu"),
                     (torch.zeros(2, 5, device="meta"), "(2, 5) torch.float32 on meta")]:
        assert refused(bare._out_buf, bad, (2, 5)) == head + got


# ------------------------------------------------------------------------------------------------------- generation bookkeeping
def test_begin_forward_bumps_what_each_entry_bumped(bare):
    """The ranges are those of the public methods on the 2-layer tower: every whole-tower walk bumps both blocks;
    ``blocks_forward(x, l_lo, l_hi)`` bumps l_lo .. min(l_hi + 1, L) - 1 (the output of block l_hi - 1 lands in the saved input
    of block l_hi); ``attention_forward`` bumps its block and records that value; the fused step bumps the tower's counter only."""
    L = bare.arch.layers
    assert L == 2
    bare._begin_forward(range(L))                                  # transformer_forward, visual_forward, predict, encode_image, zeroshot
    assert (bare.forward_generation, bare.block_generation) == (1, {0: 1, 1: 1})
    bare._begin_forward(range(0, min(1 + 1, L)))                   # blocks_forward(x, 0, 1)
    assert (bare.forward_generation, bare.block_generation) == (2, {0: 2, 1: 2})
    bare._begin_forward(range(1, min(2 + 1, L)))                   # blocks_forward(x, 1, 2)
    assert (bare.forward_generation, bare.block_generation) == (3, {0: 2, 1: 3})
    bare._begin_forward((1,), attention=True)                      # attention_forward(x, 1)
    assert (bare.forward_generation, bare.block_generation, bare.attention_generation) == (4, {0: 2, 1: 4}, {1: 4})
    bare._begin_forward((), flush=False)                           # forward_backward (the pipelined step must not flush)
    assert (bare.forward_generation, bare.block_generation, bare.attention_generation) == (5, {0: 2, 1: 4}, {1: 4})


def test_begin_forward_flushes_an_open_pipelined_step(bare, monkeypatch):
    waited = []
    bare._pipe = {"open": True, "params": "event"}
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: type("S", (), {"wait_event": waited.append})())
    bare._begin_forward((), flush=False)
    assert waited == [] and bare._pipe["open"]
    bare._begin_forward(())
    assert waited == ["event"] and not bare._pipe["open"]


# ---------------------------------------------------------------------------------------------------------------- no lazy state
MODULES = [m for m in ("engine.py", "engine_input.py", "engine_optim.py", "engine_dp.py", "_context.py", "text_engine.py")
           if os.path.exists(os.path.join(ROOT, "pevit_amd", m))]


def _trees():
    for m in MODULES:
        yield m, ast.parse(open(os.path.join(ROOT, "pevit_amd", m)).read())


def _outside_del(tree):
    """Every node of ``tree`` that is not inside a ``__del__``."""
    todo = [tree]
    while todo:
        node = todo.pop()
        if isinstance(node, ast.FunctionDef) and node.name == "__del__":
            continue
        yield node
        todo.extend(ast.iter_child_nodes(node))


def test_no_state_is_read_through_a_default():
    found = []
    for m, tree in _trees():
        for node in _outside_del(tree):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "getattr" and len(node.args) == 3 \
                    and isinstance(node.args[1], ast.Constant) and str(node.args[1].value).startswith("_"):
                found.append(f"{m}:{node.lineno} getattr(..., {node.args[1].value!r}, default)")
            if isinstance(node, ast.Attribute) and node.attr == "__dict__":
                found.append(f"{m}:{node.lineno} __dict__")
    assert not found, found


def _self_stores(fn):
    for node in ast.walk(fn):
        targets = node.targets if isinstance(node, ast.Assign) else [node.target] if isinstance(node, (ast.AugAssign, ast.AnnAssign)) else []
        for t in targets:
            for leaf in (t.elts if isinstance(t, (ast.Tuple, ast.List)) else [t]):
                if isinstance(leaf, ast.Attribute) and isinstance(leaf.value, ast.Name) and leaf.value.id == "self":
                    yield leaf.attr


def test_every_attribute_is_born_in_init():
    """A method may rebind what ``__init__`` (the class's own or a base's) declared; it introduces nothing."""
    born, later = {}, {}                       # class name -> names stored in __init__ / in any other method
    for _, tree in _trees():
        for cls in (n for n in ast.walk(tree) if isinstance(n, ast.ClassDef)):
            for fn in (n for n in cls.body if isinstance(n, ast.FunctionDef)):
                (born if fn.name == "__init__" else later).setdefault(cls.name, set()).update(_self_stores(fn))
    owners = set()
    for concrete in (HipEngine, TextEngine):
        mro = [c.__name__ for c in concrete.__mro__]
        owners.update(mro)
        declared = set().union(*(born.get(c, set()) for c in mro))
        for c in mro:
            assert later.get(c, set()) <= declared, (concrete.__name__, c, sorted(later[c] - declared))
    assert not [c for c in later if later[c] and c not in owners]            # (no other class of these modules keeps state)
