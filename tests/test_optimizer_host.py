"""CPU checks of the fused optimizer route (Adam, AdamW, SGD with several groups): the pure planner
``plan_fused_optimizer`` / ``ClassifierBase.fused_optimizer_plan`` on CPU-built Classifiers, ``can_fuse`` left as it was, the
three C-ABI entries in header and ctypes table, and the sanity of the gate the GPU tests use (tests/optim_gate.py)."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT, load_tiny_sd

import optim_gate as og
from test_mirror_api import tiny_config

from pevit_amd import _lib
from pevit_amd.engine import OptimPlan
from pevit_amd.evaluation._harness import plan_fused_optimizer
from pevit_amd.optim import build_optimizer

CE = torch.nn.CrossEntropyLoss()


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    p = tmp_path_factory.mktemp("ckpt") / "tiny.pt"
    torch.save(load_tiny_sd(), p)
    return p


def classifier(ckpt, method="kadaptation", **train):
    import importlib
    mod = importlib.import_module("pevit_amd.evaluation." + {"kadaptation": "kadaptation_clip", "adapter": "adapter_tuning_clip",
                                                             "lora": "lora_clip"}[method])
    cfg = tiny_config(ckpt)
    cfg.TRAIN.LR, cfg.TRAIN.WD = 0.1, 1e-3
    for k, v in train.items():
        setattr(cfg.TRAIN, k, v)
    return cfg, mod.Classifier(cfg, 0)


def ranges_of(clf, names):
    """element ranges of the named parameters in the flat buffer"""
    by_id = {id(p): n for n, p in clf.named_parameters()}
    return sorted((off, off + k) for p, off, k in clf._flat_layout() if by_id[id(p)] in names)


def ranges_where(group_of, value):
    idx = (group_of == value).nonzero().flatten().tolist()
    out = []
    for i in idx:
        if out and out[-1][1] == i:
            out[-1][1] = i + 1
        else:
            out.append([i, i + 1])
    return [tuple(r) for r in out]


def merged(ranges):
    out = []
    for a, b in ranges:
        if out and out[-1][1] == a:
            out[-1][1] = b
        else:
            out.append([a, b])
    return [tuple(r) for r in out]


def test_flat_layout_is_the_engine_order(ckpt):
    _, clf = classifier(ckpt)
    names = {id(p): n for n, p in clf.named_parameters()}
    order = [names[id(p)] for p, _, _ in clf._flat_layout()]
    assert order == [n for n, p in clf.named_parameters() if p.requires_grad]
    offs = [off for _, off, _ in clf._flat_layout()]
    assert offs[0] == 0 and all(b == a + k for (_, a, k), b in zip(clf._flat_layout(), offs[1:]))


@pytest.mark.parametrize("method", ["kadaptation", "adapter"])
def test_two_weight_decays_plan_the_bias_ranges(ckpt, method):
    cfg, clf = classifier(ckpt, method, WITHOUT_WD_LIST=["bias"])
    opt = build_optimizer(cfg, clf)
    plan = clf.fused_optimizer_plan(CE, opt)
    assert isinstance(plan, OptimPlan) and plan.kind == "sgd" and len(plan.groups) == 2 and plan.group_index == [0, 1]
    assert [g["weight_decay"] for g in plan.groups] == [1e-3, 0.0] and all(g["lr"] == 0.1 for g in plan.groups)
    assert plan.groups[0]["momentum"] == 0.9 and plan.groups[0]["nesterov"] is False
    bias = {n for n, p in clf.named_parameters() if p.requires_grad and n.endswith(".bias")}
    assert ranges_where(plan.group_of, 1) == merged(ranges_of(clf, bias))
    assert int((plan.group_of == 0).sum() + (plan.group_of == 1).sum()) == plan.group_of.numel()
    assert plan.group_of.dtype == torch.uint8
    assert plan.group_of.numel() == sum(p.numel() for p in clf.parameters() if p.requires_grad)
    # adjust_learning_rate keeps working: the hyper-parameters are re-read from param_groups
    for g in opt.param_groups:
        g["lr"] = 0.01
    assert [g["lr"] for g in plan.refresh(opt).groups] == [0.01, 0.01]


def test_two_learning_rates_plan_trunk_and_head(ckpt):
    cfg, clf = classifier(ckpt, TWO_LR=True)
    opt = build_optimizer(cfg, clf)
    plan = clf.fused_optimizer_plan(CE, opt)
    assert plan is not None and plan.kind == "sgd" and len(plan.groups) == 2
    assert [g["lr"] for g in plan.groups] == [pytest.approx(0.01), 0.1]
    head = {"layers.0.weight", "layers.0.bias"}
    assert ranges_where(plan.group_of, 1) == merged(ranges_of(clf, head))
    trunk = {n for n, p in clf.named_parameters() if p.requires_grad and n.startswith("backbone.")}
    assert ranges_where(plan.group_of, 0) == merged(ranges_of(clf, trunk))


@pytest.mark.parametrize("name,kind", [("adam", "adam"), ("adamW", "adamw")])
def test_adam_kinds_plan(ckpt, name, kind):
    cfg, clf = classifier(ckpt, OPTIMIZER=name, WITHOUT_WD_LIST=["bias"])
    opt = build_optimizer(cfg, clf)
    plan = clf.fused_optimizer_plan(CE, opt)
    assert plan is not None and plan.kind == kind and len(plan.groups) == 2
    assert plan.groups[0] == {"lr": 0.1, "weight_decay": 1e-3, "beta1": 0.9, "beta2": 0.999, "eps": 1e-8}
    assert plan.groups[1]["weight_decay"] == 0.0
    # one live group is planned too (only single-hyper-parameter SGD stays with can_fuse)
    cfg.TRAIN.WITHOUT_WD_LIST = []
    plan = clf.fused_optimizer_plan(CE, build_optimizer(cfg, clf))
    assert plan is not None and len(plan.groups) == 1 and plan.group_index == [0] and bool((plan.group_of == 0).all())
    assert clf.fused_optimizer_plan(torch.nn.BCEWithLogitsLoss(), build_optimizer(cfg, clf)) is not None
    assert clf.fused_optimizer_plan(torch.nn.CrossEntropyLoss(label_smoothing=0.1), build_optimizer(cfg, clf)) is None


def test_dead_v_adapters_are_marked_255(ckpt):
    """KAdaptation's v_proj_adapter1_* never receive a gradient (pevit_param_grad_mask): their ranges get 255."""
    from pevit_amd.synth import ARCHS
    cfg, clf = classifier(ckpt, OPTIMIZER="adamW")
    opt = build_optimizer(cfg, clf)
    a = ARCHS["tiny-128"]
    lib = _lib.load()
    ctx = C.c_void_p()
    d = _lib.PevitDims(a.width, a.layers, a.patch, a.resolution, a.embed_dim, _lib.METHOD_IDS["kadaptation"], 4, 10)
    assert lib.pevit_ctx_create(C.byref(d), C.byref(ctx)) == 0
    n = lib.pevit_num_params(ctx)
    m = (C.c_ubyte * n)()
    assert lib.pevit_param_grad_mask(ctx, m, n) == 0
    lib.pevit_ctx_destroy(ctx)
    mask = torch.frombuffer(bytearray(m), dtype=torch.uint8).clone()
    plan = plan_fused_optimizer(opt, clf._flat_layout(), mask)
    dead = {n for n, _ in clf.named_parameters() if "v_proj_adapter1_" in n}
    assert len(dead) == 2 * a.layers
    assert ranges_where(plan.group_of, 255) == merged(ranges_of(clf, dead))
    assert ranges_where(plan.group_of, 255) == ranges_where(mask, 0)
    # a parameter that requires a gradient but sits in no live group is left alone as well
    params = [p for p in clf.parameters() if p.requires_grad]
    opt = torch.optim.AdamW([{"params": params[:-1]}], lr=1e-3)
    plan = plan_fused_optimizer(opt, clf._flat_layout())
    assert ranges_where(plan.group_of, 255) == ranges_of(clf, {"layers.0.bias"})


def test_what_the_planner_refuses(ckpt):
    cfg, clf = classifier(ckpt)
    layout = clf._flat_layout()
    params = [p for p, _, _ in layout]
    assert clf.fused_optimizer_plan(CE, build_optimizer(cfg, clf)) is None            # plain SGD: can_fuse's case
    assert plan_fused_optimizer(build_optimizer(cfg, clf), layout) is None
    cfg.TRAIN.OPTIMIZER = "rmsprop"
    assert clf.fused_optimizer_plan(CE, build_optimizer(cfg, clf)) is None
    assert plan_fused_optimizer(torch.optim.Adam(params, lr=1e-3, amsgrad=True), layout) is None
    assert plan_fused_optimizer(torch.optim.AdamW(params, lr=1e-3, maximize=True), layout) is None
    assert plan_fused_optimizer(torch.optim.Adam(params, lr=torch.tensor(1e-3)), layout) is None
    assert plan_fused_optimizer(torch.optim.SGD([{"params": params[:3]}, {"params": params[3:], "lr": 0.1}], lr=0.01,
                                                dampening=0.1), layout) is None
    nine = [{"params": [p], "lr": 1e-3 * (i + 1)} for i, p in enumerate(params[:9])]
    assert plan_fused_optimizer(torch.optim.Adam(nine, lr=1e-3), layout) is None
    assert plan_fused_optimizer(torch.optim.Adam(nine[:8], lr=1e-3), layout) is not None
    foreign = torch.nn.Parameter(torch.zeros(3))
    assert plan_fused_optimizer(torch.optim.Adam(params + [foreign], lr=1e-3), layout) is None

    class MyAdam(torch.optim.Adam):
        pass
    assert plan_fused_optimizer(MyAdam(params, lr=1e-3), layout) is None                # exact types only


def test_fused_optimizer_key_switches_the_route_off(ckpt):
    from pevit_amd.config import default_config
    assert default_config().TRAIN.FUSED_OPTIMIZER is True
    cfg, clf = classifier(ckpt, OPTIMIZER="adamW", FUSED_OPTIMIZER=False)
    assert clf.fused_optimizer_plan(CE, build_optimizer(cfg, clf)) is None
    cfg, clf = classifier(ckpt, OPTIMIZER="adamW")
    assert clf.fused_optimizer_plan(CE, build_optimizer(cfg, clf)) is not None


def test_can_fuse_is_what_it_was(ckpt):
    """The values tests/test_mirror_api.py and tests/test_multilabel_host.py pin, and the override the GPU tests use."""
    cfg, clf = classifier(ckpt)
    bce = torch.nn.BCEWithLogitsLoss()
    opt = build_optimizer(cfg, clf)
    assert clf.can_fuse(CE, opt) and clf.can_fuse(bce, opt)
    cfg.TRAIN.NESTEROV = True
    assert clf.can_fuse(CE, build_optimizer(cfg, clf))
    cfg.TRAIN.NESTEROV = False
    cfg.TRAIN.WITHOUT_WD_LIST = ["bias"]
    two_wd = build_optimizer(cfg, clf)
    assert not clf.can_fuse(CE, two_wd) and not clf.can_fuse(bce, two_wd)
    cfg.TRAIN.WITHOUT_WD_LIST = []
    cfg.TRAIN.OPTIMIZER = "adam"
    assert not clf.can_fuse(CE, build_optimizer(cfg, clf)) and not clf.can_fuse(bce, build_optimizer(cfg, clf))
    assert not clf.can_fuse(torch.nn.CrossEntropyLoss(label_smoothing=0.1), opt)
    assert not clf.can_fuse(torch.nn.BCEWithLogitsLoss(pos_weight=torch.ones(10)), opt)
    # the autograd route forced on a plain SGD optimizer stays the autograd route: no plan takes it over
    clf.can_fuse = lambda *_: False
    assert clf.fused_optimizer_plan(CE, opt) is None


def test_abi_entries_are_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "pevit_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(pevit_(?:set_optim_state|optim_step))\s*\(([^)]*)\)", src)}
    assert sorted(decl) == ["pevit_optim_step", "pevit_set_optim_state"]
    assert re.search(r"typedef struct pevit_optim_group \{\s*double lr, weight_decay, momentum, beta1, beta2, eps;\s*int nesterov;\s*\} "
                     r"pevit_optim_group;", src)
    ctype = {"pevit_ctx*": C.c_void_p, "void*": C.c_void_p, "float*": C.c_void_p, "const unsigned char*": C.c_void_p,
             "int": C.c_int, "float": C.c_float, "const pevit_optim_group*": C.POINTER(_lib.PevitOptimGroup)}
    for name, args in decl.items():
        types = [ctype[re.sub(r"\s*\w+$", "", a.strip())] for a in args.split(",")]
        assert _lib.SIGNATURES[name] == (C.c_int, types), name
    assert [f[0] for f in _lib.PevitOptimGroup._fields_] == ["lr", "weight_decay", "momentum", "beta1", "beta2", "eps", "nesterov"]
    assert all(f[1] is C.c_double for f in _lib.PevitOptimGroup._fields_[:6]) and _lib.PevitOptimGroup._fields_[6][1] is C.c_int
    assert re.search(r"#define PEVIT_OPTIM_MAX_GROUPS 8\b", src) and _lib.OPTIM_MAX_GROUPS == 8
    assert re.search(r"PEVIT_OPTIM_SGD = 0, PEVIT_OPTIM_ADAM = 1, PEVIT_OPTIM_ADAMW = 2", src)
    assert _lib.OPTIM_KINDS == {"sgd": 0, "adam": 1, "adamw": 2}
    lib = _lib.load()
    assert hasattr(lib, "pevit_set_optim_state") and hasattr(lib, "pevit_optim_step")


def test_optim_step_refuses_bad_calls_without_a_gpu():
    """Validation happens before anything is launched: a context without parameters, then (below) nothing else can be reached
    on a CPU box -- the remaining refusals are exercised on the GPU."""
    lib = _lib.load()
    ctx = C.c_void_p()
    d = _lib.PevitDims(128, 2, 16, 48, 64, 0, 4, 10)
    assert lib.pevit_ctx_create(C.byref(d), C.byref(ctx)) == 0
    g = (_lib.PevitOptimGroup * 1)()
    assert lib.pevit_optim_step(ctx, None, 1, g, 1, 1, 1.0, 0) != 0
    assert b"parameters" in lib.pevit_last_error()
    assert lib.pevit_set_optim_state(ctx, None, None) != 0
    lib.pevit_ctx_destroy(ctx)


# ------------------------------------------------------------------------------------------------ the gate's own sanity
SHAPES = [(768, 64), (768,), (100, 512)]
MEMBERSHIP = [0, 1, 0]


@pytest.fixture(scope="module")
def gate_inputs():
    return og.make_params(SHAPES), og.make_grads(SHAPES)


@pytest.mark.parametrize("kind", ["adam", "adamw"])
def test_gate_passes_a_restatement_and_fails_eps_inside_the_root(kind, gate_inputs):
    params0, grads = gate_inputs
    p64, s64 = og.run_reference(kind, [p.double() for p in params0], grads, MEMBERSHIP, torch.float64)
    p32, s32 = og.run_reference(kind, params0, grads, MEMBERSHIP, torch.float32)
    ps, st = og.kernel_restatement(kind, params0, grads, MEMBERSHIP)
    for i in range(len(SHAPES)):
        og.gate(f"{kind} restated p[{i}]", ps[i], p32[i], p64[i])
        for k in ("exp_avg", "exp_avg_sq"):
            og.gate(f"{kind} restated {k}[{i}]", st[k][i], s32[k][i], s64[k][i])
    ps, _ = og.kernel_restatement(kind, params0, grads, MEMBERSHIP, variant="eps_in_sqrt")
    for i in range(len(SHAPES)):
        with pytest.raises(AssertionError):
            og.gate(f"{kind} eps-in-sqrt p[{i}]", ps[i], p32[i], p64[i])
