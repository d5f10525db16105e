"""The fused optimizer step for Adam, AdamW and per-group SGD (csrc/optim.hip, HipEngine.optimizer_step, the harness route
behind ClassifierBase.fused_optimizer_plan) on the GPU.

Kernel cases write gradients into ``eng.grads`` (no forward) and compare parameters and both moments with torch.optim on the CPU
under the gate of tests/optim_gate.py: dev_engine <= 4 x dev_torch per tensor, exact equality where dev_torch is 0.  tiny-128
engines: n_params is 6,026 (KAdaptation, with masked ranges in the middle) and 34,314 (Adapter) -- neither a multiple of 4 or 256;
the group boundaries at the ``.bias`` tensors fall inside blocks and inside waves (every tensor of these towers has a multiple of 4
elements but the head bias, so the only boundary off a multiple of 4 is the end of the buffer; the kernel handles one element per
lane and has no vector path that could care)."""
import ctypes as C

import pytest
import torch

from conftest import golden_param_dict, load_golden, load_tiny_sd

import optim_gate as og
from test_gpu_mirror import OneBatch, seeded_classifier

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    p = tmp_path_factory.mktemp("ckpt") / "tiny.pt"
    torch.save(load_tiny_sd(), p)
    return p


class Bench:
    """One tiny engine with its flat layout, initial parameters and seeded gradients (shared by the kernel cases)."""

    def __init__(self, method, chunks=None):
        from pevit_amd.engine import HipEngine
        from pevit_amd.synth import ARCHS
        meta, t = load_golden("tiny_" + method)
        self.t = t
        eng = HipEngine(ARCHS[meta["arch"]], meta["method"], meta["classes"], 4, lora_rank=meta["lora_r"])
        eng.load_state_dict(golden_param_dict(meta, t))
        v = eng.param_views()
        with torch.no_grad():
            v["layers.0.weight"].copy_(t["head_w"]); v["layers.0.bias"].copy_(t["head_b"])
        torch.cuda.synchronize()
        self.eng = eng
        self.names = list(v)
        self.shapes = [tuple(v[n].shape) for n in self.names]
        if chunks is not None:           # the flat buffer cut at arbitrary elements instead of at the tensors: the kernel knows no tensors
            sizes = list(chunks) + [eng.n_params - sum(chunks)]
            self.names, self.shapes = [f"chunk{i}" for i in range(len(sizes))], [(k,) for k in sizes]
        self.flat0 = eng.params.detach().cpu().clone()
        self.params0 = self.split(self.flat0)
        self.grads = og.make_grads(self.shapes, seed=11)
        mask = self.split(eng.grad_mask_host)
        self.no_grad = {i for i, m in enumerate(mask) if not bool(m.any())}
        assert eng.n_params % 256 != 0

    def split(self, flat):
        out, off = [], 0
        for s in self.shapes:
            k = 1
            for d in s:
                k *= d
            out.append(flat[off:off + k].view(s))
            off += k
        return out

    def flat(self, row):
        return torch.cat([x.reshape(-1) for x in row])

    def membership(self, grouping):
        if grouping == "one":
            return [0] * len(self.names), og.GROUP_HYPERS[:1]
        if grouping == "bias":
            return [1 if n.endswith(".bias") else 0 for n in self.names], og.GROUP_HYPERS
        half = len(self.names) // 2                         # three groups, the middle one empty
        return [0 if i < half else 2 for i in range(len(self.names))], og.THREE_GROUPS

    def plan(self, kind, membership, hypers):
        """The harness's planner on shadow Parameters laid out like the flat buffer; a single-hyper-parameter SGD is not the
        planner's business (can_fuse's case), so its plan is written by hand: the engine runs any plan."""
        from pevit_amd.engine import OptimPlan, _group_hypers
        from pevit_amd.evaluation._harness import plan_fused_optimizer
        shadow = [torch.nn.Parameter(p.clone()) for p in self.params0]
        layout, off = [], 0
        for p in shadow:
            layout.append((p, off, p.numel())); off += p.numel()
        opt = og.build_optimizer(kind, shadow, membership, hypers)
        plan = plan_fused_optimizer(opt, layout, self.eng.grad_mask_host)
        live = [(j, g) for j, g in enumerate(opt.param_groups) if g["params"]]
        if plan is None:
            assert kind.startswith("sgd") and len({(g["lr"], g["weight_decay"]) for _, g in live}) == 1
            group_of = torch.full((off,), 255, dtype=torch.uint8)
            for idx, (_, g) in enumerate(live):
                for p in g["params"]:
                    a = next(o for q, o, _ in layout if q is p)
                    group_of[a:a + p.numel()] = idx
            group_of[self.eng.grad_mask_host == 0] = 255
            plan = OptimPlan("sgd", [_group_hypers("sgd", g) for _, g in live], group_of, [j for j, _ in live])
        assert len(plan.groups) == len(live)
        return plan

    def run(self, plan, grads, grad_scale=1.0, sentinel=None):
        """(params, exp_avg / momentum, exp_avg_sq) as flat CPU tensors after stepping through ``grads``."""
        eng = self.eng
        eng.reset_optimizer()
        eng.params.copy_(self.flat0)
        if plan.kind != "sgd":
            eng._adam_state()
        if sentinel is not None:                             # recognisable bits in the state of the elements nobody may touch
            dead = (plan.group_of == 255).to(eng.device)
            eng.momentum[dead] = sentinel
            if eng.exp_avg_sq is not None:
                eng.exp_avg_sq[dead] = sentinel
        for row in grads:
            eng.grads.copy_(self.flat(row))
            eng.optimizer_step(plan, grad_scale)
        torch.cuda.synchronize()
        v = eng.exp_avg_sq.cpu().clone() if eng.exp_avg_sq is not None else None
        return eng.params.cpu().clone(), eng.momentum.cpu().clone(), v


_BENCHES = {}


def bench(method, chunks=None):
    key = (method, chunks)
    if key not in _BENCHES:
        _BENCHES[key] = Bench(method, chunks)
    return _BENCHES[key]


def check_against_torch(b, kind, membership, hypers, got, grads, label, no_grad=None):
    no_grad = b.no_grad if no_grad is None else no_grad
    p64, s64 = og.run_reference(kind, [p.double() for p in b.params0], grads, membership, torch.float64, no_grad, hypers)
    p32, s32 = og.run_reference(kind, b.params0, grads, membership, torch.float32, no_grad, hypers)
    gp, gm, gv = (b.split(x) if x is not None else None for x in got)
    keys = og.STATE_KEYS[kind]
    for i, n in enumerate(b.names):
        og.gate(f"{label} {n} p", gp[i], p32[i], p64[i])
        for key, mine in zip(keys, (gm, gv)):
            if s64[key][i] is None:
                assert i in no_grad
                continue
            og.gate(f"{label} {n} {key}", mine[i], s32[key][i], s64[key][i])


@pytest.mark.parametrize("method", ["kadaptation", "adapter"])
@pytest.mark.parametrize("grouping", ["one", "bias", "three"])
@pytest.mark.parametrize("kind", ["adam", "adamw", "sgd", "sgd_nesterov"])
def test_kernel_matches_torch_under_the_gate(kind, grouping, method):
    b = bench(method)
    membership, hypers = b.membership(grouping)
    plan = b.plan(kind, membership, hypers)
    if grouping == "bias":
        starts = ((plan.group_of[1:] != plan.group_of[:-1]).nonzero().flatten() + 1).tolist()
        assert any(s % 256 for s in starts)                # group boundaries inside a block (inside a wave: the odd-cut case below)
    sentinel = 7.0
    got = b.run(plan, b.grads, sentinel=sentinel)
    check_against_torch(b, kind, membership, hypers, got, b.grads, f"{kind}/{grouping}/{method}")
    # elements marked 255 keep their parameter and state bits
    dead = plan.group_of == 255
    assert int(dead.sum()) == sum(b.params0[i].numel() for i in b.no_grad)
    assert torch.equal(got[0][dead], b.flat0[dead])
    assert bool((got[1][dead] == sentinel).all())
    if got[2] is not None and kind in ("adam", "adamw"):
        assert bool((got[2][dead] == sentinel).all())
    if method == "kadaptation":
        assert int(dead.sum()) > 0 and 0 < int(dead.nonzero()[0]) and int(dead.nonzero()[-1]) < dead.numel() - 1


@pytest.mark.parametrize("kind", ["adam", "adamw", "sgd_nesterov"])
def test_group_boundaries_inside_a_wave(kind):
    """Every tensor of the tiny towers starts at a multiple of 64 elements, so the ``.bias`` rule never puts two groups into one
    wave there (ViT-B/32 heads with 100 classes do).  Here the Adapter buffer is cut at odd elements and the pieces alternate
    between the two groups: boundaries that are no multiple of 4, 64 or 256."""
    b = bench("adapter", (1001, 37, 131, 2047, 5001, 67, 259, 64, 9999))
    membership = [i % 2 for i in range(len(b.names))]
    plan = b.plan(kind, membership, og.GROUP_HYPERS)
    starts = ((plan.group_of[1:] != plan.group_of[:-1]).nonzero().flatten() + 1).tolist()
    assert len(starts) == len(b.names) - 1 and sum(1 for s in starts if s % 4) >= 6 and sum(1 for s in starts if s % 64) >= 8
    got = b.run(plan, b.grads)
    check_against_torch(b, kind, membership, og.GROUP_HYPERS, got, b.grads, f"{kind}/odd cuts")


@pytest.mark.parametrize("kind", ["adamw", "sgd"])
def test_grad_scale_is_applied_to_the_gradient(kind):
    """grad_scale = 0.5 on g == grad_scale = 1 on 0.5 g, bit for bit: the product is exact."""
    b = bench("kadaptation")
    membership, hypers = b.membership("bias")
    plan = b.plan(kind, membership, hypers)
    a = b.run(plan, b.grads, grad_scale=0.5)
    c = b.run(plan, [[0.5 * g for g in row] for row in b.grads], grad_scale=1.0)
    for x, y in zip(a, c):
        assert (x is None and y is None) or torch.equal(x, y)
    assert not torch.equal(a[0], b.run(plan, b.grads)[0])


@pytest.mark.parametrize("nesterov", [False, True])
def test_per_group_sgd_with_identical_groups_against_sgd_step(nesterov):
    """Two groups with the same hyper-parameters through the new kernel, and ``sgd_step`` on the same gradients: both under the
    gate (the two kernels may contract g * s + wd * p differently, so bit identity is not required).  The two are also compared
    with each other in the gate's unit: per tensor, max |optimizer_step - sgd_step| <= 4 x dev_torch (dev_torch = max |torch f32 -
    torch f64|), equal where dev_torch is 0 -- both are f32 evaluations of the one formula that differ in a few roundings, the
    reasoning behind the gate's 4."""
    b = bench("adapter")
    kind = "sgd_nesterov" if nesterov else "sgd"
    membership, _ = b.membership("bias")
    hypers = [og.GROUP_HYPERS[0], og.GROUP_HYPERS[0]]
    plan = b.plan(kind, membership, hypers)
    assert len(plan.groups) == 2 and plan.groups[0] == plan.groups[1]
    got = b.run(plan, b.grads)
    check_against_torch(b, kind, membership, hypers, got, b.grads, f"{kind}/identical groups")
    eng = b.eng
    eng.reset_optimizer()
    eng.params.copy_(b.flat0)
    for row in b.grads:
        eng.grads.copy_(b.flat(row))
        eng.sgd_step(hypers[0]["lr"], 0.9, hypers[0]["weight_decay"], 1.0, nesterov)
    torch.cuda.synchronize()
    old = (eng.params.cpu().clone(), eng.momentum.cpu().clone(), None)
    check_against_torch(b, kind, membership, hypers, old, b.grads, f"{kind}/sgd_step")
    print("max |optimizer_step - sgd_step|", float((old[0] - got[0]).abs().max()), float((old[1] - got[1]).abs().max()))
    p64, s64 = og.run_reference(kind, [p.double() for p in b.params0], b.grads, membership, torch.float64, b.no_grad, hypers)
    p32, s32 = og.run_reference(kind, b.params0, b.grads, membership, torch.float32, b.no_grad, hypers)
    key = og.STATE_KEYS[kind][0]
    for i, n in enumerate(b.names):
        for what, new, ref, t32, t64 in (("p", b.split(got[0])[i], b.split(old[0])[i], p32[i], p64[i]),
                                         (key, b.split(got[1])[i], b.split(old[1])[i], s32[key][i], s64[key][i])):
            if t64 is None:
                assert i in b.no_grad
                continue
            dev_torch = float((t32.double() - t64).abs().max())
            diff = float((new.double() - ref.double()).abs().max())
            print(f"{kind} {n} {what}: |optimizer_step - sgd_step| {diff:.3e}, dev_torch {dev_torch:.3e}")
            assert diff <= 4 * dev_torch, (n, what, diff, dev_torch)


def test_external_error_word_withholds_the_update():
    """pevit_set_external_poison on the new kernel: parameters and both moments keep their bits, the step's loss reads NaN; the
    next step after detaching the word applies."""
    from pevit_amd import _lib
    b = bench("kadaptation")
    eng = b.eng
    membership, hypers = b.membership("bias")
    plan = b.plan("adamw", membership, hypers)
    eng.reset_optimizer()
    eng.params.copy_(b.flat0)
    img, lab = b.t["images"].cuda().contiguous(), b.t["labels"].cuda().contiguous()
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(eng.lib.pevit_set_external_poison(eng._ctx, C.c_void_p(word.data_ptr())), "pevit_set_external_poison")
    try:
        _, loss = eng.train_step(img, lab, optimizer=plan)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss).all()) and not torch.equal(eng.params.cpu(), b.flat0)
        p1, m1, v1 = eng.params.clone(), eng.momentum.clone(), eng.exp_avg_sq.clone()
        word.fill_(1)
        _, loss = eng.train_step(img, lab, optimizer=plan)
        torch.cuda.synchronize()
        assert torch.equal(eng.params, p1) and torch.equal(eng.momentum, m1) and torch.equal(eng.exp_avg_sq, v1)
        assert bool(torch.isnan(loss).all())
    finally:
        _lib.check(eng.lib.pevit_set_external_poison(eng._ctx, None), "pevit_set_external_poison")
    _, loss = eng.train_step(img, lab, optimizer=plan)
    torch.cuda.synchronize()
    assert not torch.equal(eng.params, p1) and not torch.equal(eng.exp_avg_sq, v1) and bool(torch.isfinite(loss).all())


def test_engine_gradients_three_adamw_steps():
    """forward_backward on the fixture batch; the engine's own gradients go to the CPU shadow optimizers each step."""
    b = bench("kadaptation")
    eng = b.eng
    membership, hypers = b.membership("bias")
    plan = b.plan("adamw", membership, hypers)
    eng.reset_optimizer()
    eng.params.copy_(b.flat0)
    img, lab = b.t["images"].cuda().contiguous(), b.t["labels"].cuda().contiguous()
    sh64 = og.Shadow("adamw", [p.double() for p in b.params0], membership, torch.float64, b.no_grad, hypers)
    sh32 = og.Shadow("adamw", b.params0, membership, torch.float32, b.no_grad, hypers)
    for _ in range(3):
        eng.forward_backward(img, lab)
        torch.cuda.synchronize()
        row = b.split(eng.grads.cpu().clone())
        assert all(bool(torch.isfinite(g).all()) for g in row) and any(float(g.abs().max()) > 0 for g in row)
        sh64.step(row); sh32.step(row)
        eng.optimizer_step(plan)
    torch.cuda.synchronize()
    (p64, s64), (p32, s32) = sh64.result(), sh32.result()
    gp, gm, gv = b.split(eng.params.cpu()), b.split(eng.momentum.cpu()), b.split(eng.exp_avg_sq.cpu())
    for i, n in enumerate(b.names):
        og.gate(f"engine grads {n} p", gp[i], p32[i], p64[i])
        if i in b.no_grad:
            continue
        og.gate(f"engine grads {n} exp_avg", gm[i], s32["exp_avg"][i], s64["exp_avg"][i])
        og.gate(f"engine grads {n} exp_avg_sq", gv[i], s32["exp_avg_sq"][i], s64["exp_avg_sq"][i])


def test_state_belongs_to_one_kind_and_capture_refuses_plans():
    from pevit_amd import _lib
    b = bench("kadaptation")
    eng = b.eng
    membership, hypers = b.membership("bias")
    adamw, adam, sgd = (b.plan(k, membership, hypers) for k in ("adamw", "adam", "sgd"))
    eng.reset_optimizer()
    eng.params.copy_(b.flat0)
    eng.grads.copy_(b.flat(b.grads[0]))
    eng.optimizer_step(adamw)
    for other in (adam, sgd):
        with pytest.raises(_lib.PevitError, match="reset_optimizer"):
            eng.optimizer_step(other)
    with pytest.raises(_lib.PevitError, match="reset_optimizer"):
        eng.sgd_step(0.01)
    eng.optimizer_step(adamw)                                   # the refusals changed nothing
    assert eng._steps == 2
    img, lab = b.t["images"].cuda().contiguous(), b.t["labels"].cuda().contiguous()
    with pytest.raises(_lib.PevitError, match="plain-SGD"):
        eng.capture_train_step(img, lab, optimizer=adamw)
    eng.reset_optimizer()
    assert float(eng.momentum.abs().max()) == 0.0 and float(eng.exp_avg_sq.abs().max()) == 0.0
    eng.optimizer_step(sgd)                                     # after a reset another kind is welcome
    with pytest.raises(_lib.PevitError, match="reset_optimizer"):
        eng.optimizer_step(adam)
    eng.reset_run()
    assert float(eng.exp_avg_sq.abs().max()) == 0.0 and eng._optim_kind is None
    torch.cuda.synchronize()


def test_abi_refuses_bad_calls_and_launches_nothing():
    from pevit_amd import _lib
    from pevit_amd.engine import HipEngine
    from pevit_amd.synth import ARCHS
    eng = HipEngine(ARCHS["tiny-128"], "lora", 10, 4)
    eng.params.fill_(1.0); eng.grads.fill_(1.0)
    lib, s = eng.lib, _lib.stream_ptr()
    g = (_lib.PevitOptimGroup * 9)()
    for h in g:
        h.lr, h.beta1, h.beta2, h.eps = 1e-3, 0.9, 0.999, 1e-8
    assert lib.pevit_optim_step(eng._ctx, s, 1, g, 1, 1, 1.0, 1) != 0 and b"state not set" in lib.pevit_last_error()
    group_of = torch.zeros(eng.n_params, dtype=torch.uint8, device="cuda")
    assert lib.pevit_set_optim_state(eng._ctx, None, _lib.ptr(group_of)) == 0
    assert lib.pevit_optim_step(eng._ctx, s, 2, g, 1, 1, 1.0, 1) != 0 and b"state not set" in lib.pevit_last_error()   # Adam kinds need exp_avg_sq
    v = torch.zeros_like(eng.params)
    assert lib.pevit_set_optim_state(eng._ctx, _lib.ptr(v), _lib.ptr(group_of)) == 0
    for n_groups in (0, 9, -1):
        assert lib.pevit_optim_step(eng._ctx, s, 1, g, n_groups, 1, 1.0, 1) != 0 and b"parameter groups" in lib.pevit_last_error()
    assert lib.pevit_optim_step(eng._ctx, s, 1, g, 1, 0, 1.0, 1) != 0 and b"count updates from 1" in lib.pevit_last_error()
    assert lib.pevit_optim_step(eng._ctx, s, 3, g, 1, 1, 1.0, 1) != 0 and b"unknown optimizer kind" in lib.pevit_last_error()
    torch.cuda.synchronize()
    assert bool((eng.params == 1.0).all()) and float(v.abs().max()) == 0.0 and float(eng.momentum.abs().max()) == 0.0
    assert lib.pevit_optim_step(eng._ctx, s, 0, g, 8, 0, 1.0, 1) == 0       # SGD kind: any step count, 8 groups
    assert lib.pevit_optim_step(eng._ctx, s, 1, g, 1, 1, 1.0, 1) == 0
    torch.cuda.synchronize()
    assert bool((eng.params != 1.0).all())


# ------------------------------------------------------------------------------------------------------------------- harness
@pytest.mark.parametrize("over", [dict(OPTIMIZER="adamW", WITHOUT_WD_LIST=["bias"]), dict(OPTIMIZER="sgd", TWO_LR=True)],
                         ids=["adamW-two-wd", "sgd-two-lr"])
def test_train_one_takes_the_fused_route_bit_for_bit(over, ckpt):
    """train_one over three batches == the same three HipEngine.train_step(..., optimizer=plan) calls made by hand; the torch
    optimizer's own state stays empty (the moments live in the engine)."""
    meta, t = load_golden("tiny_kadaptation")
    crit = torch.nn.CrossEntropyLoss().cuda(0)
    mod, cfg, clf = seeded_classifier("kadaptation", ckpt, meta, t, NESTEROV=False, **over)
    opt = mod.build_optimizer(cfg, clf)
    assert not clf.can_fuse(crit, opt) and clf.fused_optimizer_plan(crit, opt) is not None
    mod.train_one(OneBatch(t["images"], t["labels"], 3), clf, crit, opt, 0, cfg)
    torch.cuda.synchronize()
    eng = clf.engine()
    assert len(opt.state) == 0 and eng._steps == 3 and eng._optim_kind == ("adamw" if over["OPTIMIZER"] == "adamW" else "sgd")
    assert int(clf.channel_bn.num_batches_tracked) == 3
    got = [x.detach().cpu().clone() for x in (eng.params, eng.momentum, eng.running_mean, eng.running_var)]
    got_v = eng.exp_avg_sq.cpu().clone() if over["OPTIMIZER"] == "adamW" else None
    assert not torch.equal(got[0], torch.zeros_like(got[0]))
    del clf, opt

    mod, cfg, clf = seeded_classifier("kadaptation", ckpt, meta, t, NESTEROV=False, **over)
    opt = mod.build_optimizer(cfg, clf)
    eng = clf.engine()
    plan = clf.fused_optimizer_plan(crit, opt)
    # the layout the plan was made over is the engine's buffer: every module parameter is the view at its offset, none is missed
    layout = clf._flat_layout()
    for p, off, k in layout:
        assert p.data_ptr() == eng.params.data_ptr() + 4 * off and p.numel() == k
    assert sum(k for _, _, k in layout) == eng.n_params
    by_name = {id(p): n for n, p in clf.named_parameters()}
    for j, grp in zip(plan.group_index, range(len(plan.groups))):
        for q in opt.param_groups[j]["params"]:
            if q.requires_grad:
                off = next(o for r, o, _ in layout if r is q)
                want_g = 255 if "v_proj_adapter1" in by_name[id(q)] else grp
                assert bool((plan.group_of[off:off + q.numel()] == want_g).all()), by_name[id(q)]
    before = eng.params.cpu().clone()
    img, lab = t["images"].cuda(0).contiguous().float(), t["labels"].cuda(0).contiguous()
    for _ in range(3):
        eng.train_step(img, lab, bn_training=True, optimizer=plan)
    torch.cuda.synchronize()
    want = [x.detach().cpu().clone() for x in (eng.params, eng.momentum, eng.running_mean, eng.running_var)]
    assert not torch.equal(want[0], before)
    for a, w in zip(got, want):
        assert torch.equal(a, w)
    if got_v is not None:
        assert torch.equal(got_v, eng.exp_avg_sq.cpu())
    # the dead v adapters and their state never moved
    dead = plan.group_of == 255
    assert int(dead.sum()) > 0 and torch.equal(want[0][dead], before[dead]) and float(want[1][dead].abs().max()) == 0.0


def test_fused_optimizer_false_restores_the_torch_route(ckpt):
    meta, t = load_golden("tiny_kadaptation")
    crit = torch.nn.CrossEntropyLoss().cuda(0)
    mod, cfg, clf = seeded_classifier("kadaptation", ckpt, meta, t, OPTIMIZER="adamW", WITHOUT_WD_LIST=["bias"],
                                      FUSED_OPTIMIZER=False)
    opt = mod.build_optimizer(cfg, clf)
    assert clf.fused_optimizer_plan(crit, opt) is None
    before = clf.engine().params.cpu().clone()
    mod.train_one(OneBatch(t["images"], t["labels"], 3), clf, crit, opt, 0, cfg)
    torch.cuda.synchronize()
    eng = clf.engine()
    assert len(opt.state) > 0 and all(int(s["step"]) == 3 for s in opt.state.values())
    assert eng._steps == 0 and eng._optim_kind is None             # the engine's optimizer never ran
    assert not torch.equal(eng.params.cpu(), before)
