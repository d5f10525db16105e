"""Gradient-norm clipping on the GPU (csrc/clip.hip): the two launches alone -- the norm against f64 under the bound of blocked f32
summation, the scaling bit for bit, determinism, the ticket, the numeric edges --, then inside the step on the tiny towers, under
``grad_scale``, captured into a graph, in the linear probe's ``train_one``, and counted launch by launch.

Gate 1, the norm: |total - norm_f64| <= (ceil(log2 n) + 3) * 2^-24 * norm_f64.  Every f32 rounding is at most 2^-24 relative; a
blocked summation of n positive terms puts at most ceil(log2 n) + O(1) of them on any path from a square to the sum, the square
root halves the relative error of the sum, and three more roundings follow (the square root, the product with grad_scale, f64 to
f32).  Measured maxima over the buffers of this file: profiles/grad_clip.md."""
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch
from torch import nn

from conftest import FLOOR_C, ROOT, max_rel

from pevit_amd import _lib

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CHUNK = int(re.search(r"constexpr int CLIP_CHUNK = (\d+);", open(os.path.join(ROOT, "pevit_amd", "csrc", "kernels.h")).read()).group(1))
GUARD = 32                        # sentinel elements on either side of every buffer a launch writes


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def lib():
    yield _lib.load()
    if _WORST["engine"]:                                    # the measured maxima of section 1, for profiles/grad_clip.md
        print(f"\nlargest error over gate 1: engine {_WORST['engine']:.3f}, torch f32 clip_grad_norm_ {_WORST['torch']:.3f}")


def gate1(n):
    return (math.ceil(math.log2(n)) + 3) * U


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a.cpu()), bits(b.cpu()))


def spread(n, seed):
    """gaussian values whose magnitudes are spread over 1e-6 ... 1e3"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 9.0 - 6.0)


def coef_of(total, max_norm):
    """clip_grad_norm_'s coefficient in torch f32 (on the host: IEEE division) from a given total"""
    return torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (total.cpu().float() + 1e-6), max=1.0)


class Launch:
    """One buffer (and mask) between guard elements on the device, a zeroed scratch, and the launch pair on them."""

    def __init__(self, lib, values, mask=None):
        self.lib, self.n = lib, values.numel()
        self.whole = torch.full((self.n + 2 * GUARD,), -7.25, dtype=torch.float32, device="cuda")
        self.g = self.whole[GUARD:GUARD + self.n]
        self.g.copy_(values)
        self.mwhole = self.m = None
        if mask is not None:
            self.mwhole = torch.full((self.n + 2 * GUARD,), 1, dtype=torch.uint8, device="cuda")
            self.m = self.mwhole[GUARD:GUARD + self.n]
            self.m.copy_(mask)
        self.scratch = torch.zeros(lib.pevit_clip_scratch_floats(self.n) + GUARD, dtype=torch.float32, device="cuda")
        self.scratch[-GUARD:] = -7.25

    def __call__(self, max_norm, grad_scale=1.0):
        rc = self.lib.pevit_op_clip_grad_norm(_lib.stream_ptr(), _lib.ptr(self.g), _lib.ptr(self.m), self.n, max_norm, grad_scale,
                                              _lib.ptr(self.scratch))
        assert rc == 0, self.lib.pevit_last_error()
        torch.cuda.synchronize()
        for w in (self.whole[:GUARD], self.whole[-GUARD:], self.scratch[-GUARD:]):
            assert bool((w == -7.25).all()), "a launch wrote outside its buffer"
        assert int(bits(self.scratch[2:3]).item()) == 0, "the ticket is not back at zero"
        return self.scratch[0].cpu(), self.scratch[1].cpu(), self.g.cpu().clone()


# ---- 1. the kernels: norm and bit-exact scaling ---------------------------------------------------------------------------------
SIZES = [1, 3, 63, 64, 65, 1023, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5, 2 ** 20 + 3]
_WORST = {"engine": 0.0, "torch": 0.0}


@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
@pytest.mark.parametrize("n", SIZES)
def test_norm_under_the_gate_and_scaling_bit_for_bit(lib, n, masked):
    before = spread(n, seed=n)
    mask = None
    if masked:
        mask = (torch.rand(n, generator=torch.Generator().manual_seed(n + 1)) < 0.75).to(torch.uint8)
    live = torch.ones(n, dtype=torch.bool) if mask is None else mask.bool()
    ref = float(before.double()[live].square().sum().sqrt())
    for factor in (0.5, 2.0):                               # max_norm below and above the norm
        max_norm = float(torch.tensor(ref * factor, dtype=torch.float32)) if ref else 1.0
        run = Launch(lib, before, mask)
        total, coef, after = run(max_norm)
        err = abs(float(total) - ref) / ref if ref else abs(float(total))
        _WORST["engine"] = max(_WORST["engine"], err / gate1(n))
        if mask is None:                                    # torch's own f32 norm of the same buffer, for the record
            p = nn.Parameter(torch.zeros(n, device="cuda")); p.grad = before.cuda()
            t = float(torch.nn.utils.clip_grad_norm_([p], 1e30))
            _WORST["torch"] = max(_WORST["torch"], abs(t - ref) / ref / gate1(n))
            print(f"n {n}: engine {err / U:.2f} u, torch f32 {abs(t - ref) / ref / U:.2f} u, gate {gate1(n) / U:.0f} u")
        assert err <= gate1(n), f"n {n}: total {float(total)!r} vs {ref!r}: {err / U:.2f} u over the gate {gate1(n) / U:.0f} u"
        want = coef_of(total, max_norm)
        assert same_bits(coef, want), (float(coef), float(want))
        if ref > 1e-3:                                      # (under that the 1e-6 of the formula decides)
            assert (float(want) == 1.0) == (factor == 2.0)
        assert same_bits(after, torch.where(live, before * want, before)), f"n {n} max_norm {max_norm}: scaled buffer"
        # the same buffer once more, on the scratch the first call left behind: equal bits everywhere
        run.g.copy_(before)
        total2, coef2, after2 = run(max_norm)
        assert same_bits(total, total2) and same_bits(coef, coef2) and same_bits(after, after2)


# ---- 2. edges ---------------------------------------------------------------------------------------------------------------------
EDGE_N = CHUNK + 77


def test_all_zeros(lib):
    total, coef, after = Launch(lib, torch.zeros(EDGE_N))(1.0)
    assert float(total) == 0.0 and float(coef) == 1.0 and same_bits(after, torch.zeros(EDGE_N))


def test_norm_equal_to_the_bound_and_just_below_it(lib):
    before = torch.zeros(EDGE_N)
    at = torch.randperm(EDGE_N, generator=torch.Generator().manual_seed(5))[:1024]
    before[at] = 2.5                                        # 1024 * 6.25 = 80^2, every sum exact
    before[at[0]] = -2.5
    for max_norm in (80.0, float(torch.nextafter(torch.tensor(80.0), torch.tensor(math.inf)))):
        total, coef, after = Launch(lib, before)(max_norm)
        assert float(total) == 80.0 and float(coef) == 1.0 and same_bits(after, before), max_norm
    total, coef, after = Launch(lib, before)(float(torch.nextafter(torch.tensor(80.0), torch.tensor(0.0))))
    assert float(coef) < 1.0 and same_bits(after, before * coef_of(total, float(torch.nextafter(torch.tensor(80.0), torch.tensor(0.0)))))


def test_denormals(lib):
    g = torch.Generator().manual_seed(9)
    before = (torch.randint(1, 2 ** 22, (EDGE_N,), generator=g, dtype=torch.int32)).view(torch.float32).clone()      # all subnormal
    before[::3] *= -1.0
    assert bool((before.abs() < 1.1754944e-38).all()) and bool((before != 0).all())
    total, coef, after = Launch(lib, before)(1.0)
    assert float(total) == 0.0 and float(coef) == 1.0 and same_bits(after, before)          # their squares underflow, as in torch f32
    total, coef, after = Launch(lib, before)(1e-7)                                           # coef = 1e-7 / 1e-6: subnormal products
    assert same_bits(coef, coef_of(total, 1e-7)) and 0.09 < float(coef) < 0.11
    assert same_bits(after, before * coef)


def test_one_nan_poisons_every_counted_element(lib):
    before = spread(EDGE_N, seed=3)
    before[CHUNK + 5] = math.nan
    mask = torch.ones(EDGE_N, dtype=torch.uint8); mask[10:20] = 0
    total, coef, after = Launch(lib, before, mask)(1.0)
    assert math.isnan(float(total)) and math.isnan(float(coef))
    assert bool(after[mask.bool()].isnan().all()) and same_bits(after[10:20], before[10:20])


def test_one_inf_zeroes_the_finite_elements(lib):
    before = spread(EDGE_N, seed=4)
    before[100] = math.inf
    total, coef, after = Launch(lib, before)(1.0)
    assert float(total) == math.inf and float(coef) == 0.0
    finite = torch.ones(EDGE_N, dtype=torch.bool); finite[100] = False
    assert same_bits(after[finite], torch.copysign(torch.zeros(EDGE_N), before)[finite]) and math.isnan(float(after[100]))


def test_a_masked_nan_does_not_reach_the_norm(lib):
    before = spread(EDGE_N, seed=6)
    mask = torch.ones(EDGE_N, dtype=torch.uint8)
    for i in (0, 4097, EDGE_N - 1):
        before[i] = math.nan; mask[i] = 0
    ref = float(before.double()[mask.bool()].square().sum().sqrt())
    total, coef, after = Launch(lib, before, mask)(ref / 2)
    assert abs(float(total) - ref) <= gate1(EDGE_N) * ref and same_bits(coef, coef_of(total, ref / 2))
    assert same_bits(after, torch.where(mask.bool(), before * coef, before))


# ---- 3. the step on the tiny towers ---------------------------------------------------------------------------------------------------
HYPER = dict(lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)


def step_data(b, bce):
    img, lab = b.t["images"].cuda().contiguous(), b.t["labels"].cuda().contiguous()
    if bce:
        g = torch.Generator().manual_seed(21)
        lab = (torch.rand((img.shape[0], b.eng.num_classes), generator=g) < 0.3).float().cuda()
    return img, lab


def fresh(b, sentinel=None):
    eng = b.eng
    eng.reset_run()
    eng.params.copy_(b.flat0)
    if sentinel is not None:
        eng.momentum[eng.grad_mask == 0] = sentinel
    torch.cuda.synchronize()
    return eng


def clipped_step(eng, bound, img, lab, **kw):
    """``train_step`` under ``eng.max_grad_norm = bound`` (None: off); the attribute is put back to None"""
    eng.max_grad_norm = bound
    try:
        return eng.train_step(img, lab, **kw)
    finally:
        eng.max_grad_norm = None


def snapshot(eng, logits, loss):
    torch.cuda.synchronize()
    out = dict(logits=logits.clone(), loss=loss.clone(), params=eng.params.clone(), momentum=eng.momentum.clone(),
               grads=eng.grads.clone(), mean=eng.running_mean.clone(), var=eng.running_var.clone())
    if eng.exp_avg_sq is not None:
        out["exp_avg_sq"] = eng.exp_avg_sq.clone()
    return out


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert same_bits(a[k], b[k]), f"{what}: {k} differs"


def two_group_adamw(b):
    membership, hypers = b.membership("bias")
    return b.plan("adamw", membership, hypers)


@pytest.mark.parametrize("optimizer", ["sgd", "adamw2"])
@pytest.mark.parametrize("bce", [False, True], ids=["ce", "bce"])
@pytest.mark.parametrize("method", ["kadaptation", "adapter"])
def test_clipped_step_is_backward_then_torch_scaling_then_the_same_update(method, bce, optimizer):
    from test_gpu_optimizer import bench
    b = bench(method)
    img, lab = step_data(b, bce)
    plan = two_group_adamw(b) if optimizer == "adamw2" else None
    kw = dict(optimizer=plan) if plan is not None else HYPER
    live = b.eng.grad_mask.bool()
    # a bound that binds: half the norm of the first step's gradients
    eng = fresh(b)
    eng.forward_backward(img, lab)
    bound = float(eng.grads[live].double().square().sum().sqrt()) / 2
    # A: the clipped step, twice (the first-step flag, then the momentum)
    eng = fresh(b, sentinel=123.5)
    A, norms, coefs = [], [], []
    for _ in range(2):
        logits, loss = clipped_step(eng, bound, img, lab, **kw)
        A.append(snapshot(eng, logits, loss))
        norms.append(eng.last_grad_norm.cpu().clone()); coefs.append(eng._clip_scratch[1].cpu().clone())
    # B: the same from its parts, the scaling by torch with the coefficient torch's formula gives for the engine's total
    eng = fresh(b, sentinel=123.5)
    for step in range(2):
        logits, loss = eng.forward_backward(img, lab)
        torch.cuda.synchronize()
        ps = []
        for v in eng.grad_views().values():                     # torch's own clip of the same gradients: the norm it reports
            ps.append(nn.Parameter(torch.zeros_like(v))); ps[-1].grad = v.clone()
        torch_total = float(torch.nn.utils.clip_grad_norm_(ps, bound))
        assert abs(float(norms[step]) - torch_total) <= gate1(eng.n_params) * torch_total, (step, float(norms[step]), torch_total)
        coef = coef_of(norms[step], bound)
        assert same_bits(coef, coefs[step]) and float(coef) < 1.0
        eng.grads.mul_(torch.where(live, coef.cuda(), torch.ones((), device="cuda")))
        if plan is not None:
            eng.optimizer_step(plan)
        else:
            eng.sgd_step(**HYPER)
        assert_same(A[step], snapshot(eng, logits, loss), f"{method} step {step}")
    # the tensors torch gives no gradient stay as they were: zero gradient, the sentinel in their momentum, their parameters
    dead = ~live
    if bool(dead.any()):
        assert method == "kadaptation"
        assert same_bits(eng.grads[dead], torch.zeros(int(dead.sum()))) and bool((eng.momentum[dead] == 123.5).all())
        assert same_bits(eng.params[dead], b.flat0.cuda()[dead])


@pytest.mark.parametrize("optimizer", ["sgd", "adamw2"])
@pytest.mark.parametrize("method", ["kadaptation", "adapter"])
def test_a_bound_far_above_the_norm_changes_no_bit(method, optimizer):
    from test_gpu_optimizer import bench
    b = bench(method)
    img, lab = step_data(b, False)
    plan = two_group_adamw(b) if optimizer == "adamw2" else None
    kw = dict(optimizer=plan) if plan is not None else HYPER
    runs = []
    for bound in (None, 1e9):
        eng, steps = fresh(b), []
        for _ in range(2):
            logits, loss = clipped_step(eng, bound, img, lab, **kw)
            steps.append(snapshot(eng, logits, loss))
        runs.append(steps)
    assert float(b.eng._clip_scratch[1]) == 1.0 and float(b.eng.last_grad_norm) > 0.0
    for step in range(2):
        assert_same(runs[0][step], runs[1][step], f"{method} {optimizer} step {step}")


# ---- 4. grad_scale: the sum of two shards at 1/2 is the clip of their average ----------------------------------------------------------
def test_grad_scale_clips_by_the_norm_of_the_average(lib):
    n = 3 * CHUNK + 5
    g1, g2 = (torch.randn(n, generator=torch.Generator().manual_seed(s)) for s in (31, 32))
    mask = (torch.rand(n, generator=torch.Generator().manual_seed(33)) < 0.9).to(torch.uint8)
    summed = g1 + g2
    bound = float(torch.tensor(float((summed.double() * 0.5)[mask.bool()].square().sum().sqrt()) / 3, dtype=torch.float32))
    t_sum, c_sum, a_sum = Launch(lib, summed, mask)(bound, 0.5)
    t_avg, c_avg, a_avg = Launch(lib, summed * 0.5, mask)(bound, 1.0)
    assert float(c_avg) < 1.0
    assert same_bits(t_sum, t_avg) and same_bits(c_sum, c_avg)        # exact: 1/2 is a power of two
    assert same_bits(a_sum * 0.5, a_avg)                               # the buffer is scaled by coef alone; the update applies 1/2


def test_the_engine_call_scales_the_norm_only():
    from pevit_amd.engine_optim import clip_grad_norm
    from test_gpu_optimizer import bench
    b = bench("kadaptation")
    eng = fresh(b)
    eng.grads.copy_(torch.randn(eng.n_params, generator=torch.Generator().manual_seed(41)))
    before = eng.grads.clone()
    live = eng.grad_mask.bool()
    ref = float(before[live].double().square().sum().sqrt())
    total = clip_grad_norm(eng, ref / 8, grad_scale=0.5)
    torch.cuda.synchronize()
    assert total is eng.last_grad_norm and abs(float(total) - ref / 2) <= gate1(eng.n_params) * ref / 2
    coef = coef_of(total, ref / 8)
    assert same_bits(eng.grads, torch.where(live, before * coef.cuda(), before))


# ---- 5. captured ------------------------------------------------------------------------------------------------------------------------
def test_a_captured_clipped_step_replays_the_eager_bits():
    from test_gpu_optimizer import bench
    b = bench("kadaptation")
    img, lab = step_data(b, False)
    eng = fresh(b)
    eng.forward_backward(img, lab)
    bound = float(eng.grads.double().square().sum().sqrt()) / 50       # binds on every step: the norm falls from step to step
    eng = fresh(b)
    eager = []
    for _ in range(3):
        logits, loss = clipped_step(eng, bound, img, lab, **HYPER)
        eager.append(dict(snapshot(eng, logits, loss), norm=eng.last_grad_norm.clone(), coef=eng._clip_scratch[1].clone()))
    eng = fresh(b)
    clipped_step(eng, bound, img, lab, **HYPER)
    eng.max_grad_norm = bound                                   # read at capture time: the bound is baked into the graph
    replay = eng.capture_train_step(img, lab, **HYPER)
    eng.max_grad_norm = None
    for step in (1, 2):
        logits, loss = replay()
        got = dict(snapshot(eng, logits, loss), norm=eng.last_grad_norm.clone(), coef=eng._clip_scratch[1].clone())
        assert float(got["coef"]) < 1.0
        assert_same(eager[step], got, f"replay {step}")


# ---- 6. the linear probe's train_one ----------------------------------------------------------------------------------------------------
PD, PC, PROWS, PBATCH = 64, 5, 24, 8


class ProbeModel(nn.Module):
    """What full_model_finetune.train_one reads of its Classifier, over cached rows: a real engine for the engine routes, the
    torch head for the autograd route."""

    def __init__(self, route, eng, make_opt):
        super().__init__()
        g = torch.Generator().manual_seed(50)
        self.layers = nn.Sequential(nn.Linear(PD, PC))
        with torch.no_grad():
            self.layers[0].weight.copy_(torch.randn(PC, PD, generator=g) * PD ** -0.5)
            self.layers[0].bias.copy_(torch.randn(PC, generator=g) * 0.2)
        self.channel_bn = nn.BatchNorm1d(PD, affine=False)
        self.cuda()
        self.cache = SimpleNamespace(feats=(torch.randn(PROWS, PD, generator=g) * 1.5 + 0.3).cuda(),
                                     labels=torch.randint(0, PC, (PROWS,), generator=g).cuda())
        self.route, self.eng = route, eng
        self.opt = make_opt(self.layers[0])
        self.plan = None
        if route != "autograd":
            from pevit_amd.evaluation._harness import plan_fused_optimizer
            eng.reset_run()
            v = eng.param_views()
            with torch.no_grad():
                v["layers.0.weight"].copy_(self.layers[0].weight); v["layers.0.bias"].copy_(self.layers[0].bias)
            if route == "plan":
                w, bias = self.layers[0].weight, self.layers[0].bias
                self.plan = plan_fused_optimizer(self.opt, [(w, 0, w.numel()), (bias, w.numel(), bias.numel())])
                assert self.plan is not None

    def cached(self, loader):
        return self.cache

    def probe_route(self, criterion, optimizer, cache):
        return self.route, self.plan

    def engine(self):
        return self.eng

    def scale(self):
        return 1.0

    def head(self, feature):
        return self.layers(self.channel_bn(feature))

    def flush_bn_counter(self, *_):
        pass

    def head_params(self):
        if self.route == "autograd":
            return torch.cat([self.layers[0].weight.detach().reshape(-1), self.layers[0].bias.detach().reshape(-1)])
        return self.eng.params.clone()


class ProbeLoader:
    dataset = range(PROWS)

    def __len__(self):
        return PROWS // PBATCH

    def iter_indices(self):
        return iter(torch.arange(PROWS).split(PBATCH))


def probe_epoch(route, make_opt, clip):
    from pevit_amd.config import default_config
    from pevit_amd.evaluation import full_model_finetune as fmf
    from test_gpu_probe import _engine
    cfg = default_config()
    cfg.DATASET.NUM_CLASSES = PC
    cfg.TRAIN.CLIP_GRAD_NORM = clip
    model = ProbeModel(route, _engine(PD, PC), make_opt)
    fmf.train_one(ProbeLoader(), model, nn.CrossEntropyLoss(), model.opt, 0, cfg)
    torch.cuda.synchronize()
    return model


@pytest.mark.parametrize("route", ["fused", "plan"])
def test_probe_routes_follow_the_autograd_route_under_a_binding_bound(route):
    if route == "fused":
        def make_opt(lin):
            return torch.optim.SGD(lin.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-3, nesterov=True)
    else:
        def make_opt(lin):
            return torch.optim.AdamW(lin.parameters(), lr=1e-3, weight_decay=1e-2)
    devs = {}
    for clip in (0.0, 0.05):
        ref = probe_epoch("autograd", make_opt, clip)
        got = probe_epoch(route, make_opt, clip)
        devs[clip] = max_rel(got.head_params(), ref.head_params())
        if clip:
            assert float(got.eng.last_grad_norm) > clip and float(got.eng._clip_scratch[1]) < 1.0      # the bound binds
    gate = max(FLOOR_C * devs[0.0], gate1(PD * PC + PC))
    print(f"{route}: three steps, parameters against the autograd route: {devs[0.0]:.3e} unclipped, {devs[0.05]:.3e} clipped, gate {gate:.3e}")
    assert devs[0.05] <= gate


# ---- 7. launches --------------------------------------------------------------------------------------------------------------------------
def test_clipping_adds_exactly_two_launches_and_none_when_off():
    from test_gpu_optimizer import bench
    b = bench("kadaptation")
    img, lab = step_data(b, False)
    eng = fresh(b)
    eng.train_step(img, lab, **HYPER)

    def count(fn):
        _, _, gemms = eng.profile_gemms(fn, all_kernels=True)
        return gemms + sum(v[0] for v in eng.last_profile_hbm.values()), dict(eng.last_profile_hbm)

    def parts():                                            # the step as it was before the keyword existed
        eng.forward_backward(img, lab)
        eng.sgd_step(**HYPER)
    before, _ = count(parts)
    off, kinds_off = count(lambda: eng.train_step(img, lab, **HYPER))
    on, kinds_on = count(lambda: clipped_step(eng, 1.0, img, lab, **HYPER))
    assert off == before and on == off + 2
    sumsq, scale = "12", "13"                               # PEVIT_PROF_GRAD_SUMSQ, PEVIT_PROF_GRAD_SCALE: kinds the engine has no name for
    assert sumsq not in kinds_off and scale not in kinds_off
    assert kinds_on[sumsq][0] == 1 and kinds_on[scale][0] == 1


# ---- 8. the three DP schedules, on a one-rank group: the clip sits behind the exchange, in front of the update --------------------------
@pytest.mark.parametrize("mode", ["single", "staged", "pipelined"])
def test_dp_schedules_clip_between_the_exchange_and_the_update(mode, tmp_path):
    import torch.distributed as dist
    from pevit_amd.engine_optim import clip_grad_norm
    from test_gpu_optimizer import bench
    b = bench("kadaptation")
    img, lab = step_data(b, False)
    eng = fresh(b)
    eng.forward_backward(img, lab)
    bound = float(eng.grads.double().square().sum().sqrt()) / 50
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/group", rank=0, world_size=1)
    try:
        # the same step from its parts: the schedule's own forward/backward + exchange (pipelined: the fused call), clip, update
        eng = fresh(b)
        want = []
        for _ in range(2):
            if mode == "pipelined":
                logits, loss = eng.forward_backward(img, lab)
            else:
                logits, loss = eng.forward_backward_dp(img, lab, True, None, mode)
            clip_grad_norm(eng, bound, 1.0)
            eng.sgd_step(**HYPER)
            want.append(dict(snapshot(eng, logits, loss), norm=eng.last_grad_norm.clone(), coef=eng._clip_scratch[1].clone()))
        eng = fresh(b)
        eng.dp_exchange_mode = mode
        eng.max_grad_norm = bound
        for step in range(2):
            logits, loss = eng._train_step_dp(img, lab, HYPER["lr"], HYPER["momentum"], HYPER["weight_decay"], True, None, 1,
                                              HYPER["nesterov"], None, None, None)
            eng.dp_flush()
            got = dict(snapshot(eng, logits, loss), norm=eng.last_grad_norm.clone(), coef=eng._clip_scratch[1].clone())
            assert float(got["coef"]) < 1.0
            assert_same(want[step], got, f"{mode} step {step}")
    finally:
        eng.max_grad_norm = None
        eng.dp_pipeline_off()
        eng.dp_exchange_mode = "single"
        if eng._dp_streamk_off:
            eng.tune("gemm_streamk", 1); eng._dp_streamk_off = False
        dist.destroy_process_group()
