"""The gate of the fused optimizer tests (tests/test_optimizer_host.py, tests/test_gpu_optimizer.py), in one place.

Reference: ``torch.optim`` on the CPU with ``foreach=False`` on the SAME gradient tensors, run once in float64 from the f64
copies of the initial parameters and once in float32.  Per tensor ``dev_torch = max|x_f32 - x_f64|`` and
``dev_engine = max|x_engine - x_f64|`` for the parameter and for each moment in the optimizer's ``state``; the condition is
``dev_engine <= 4 * dev_torch``, and exact equality with the f32 run where ``dev_torch`` is 0.

Why 4: both sides are f32 evaluations of one formula that differ in a few roundings (lerp order, FMA contraction).  On shapes
(768,64), (768,) and (100,512) over 5 steps a torch restatement of the kernel's operation order reads 1.0 to 1.22 x dev_torch,
while wrong variants read far above 4: eps inside the square root or scaled with bc2 >= 6,000 x, a missing bc2 >= 300,000 x,
AdamW with coupled decay >= 30,000 x (test_optimizer_host.py keeps the first two statements honest).

Inputs that make those differences visible and keep the reference inside the cap: gradients N(0,1) * 10^U(-10,0) per element with
5 % exact zeros from a seeded generator, 5 steps, groups (lr 1e-4, wd 1e-2) and (lr 1e-3, wd 0)."""
import torch

GATE = 4.0
STEPS = 5
GROUP_HYPERS = [dict(lr=1e-4, weight_decay=1e-2), dict(lr=1e-3, weight_decay=0.0)]
THREE_GROUPS = [GROUP_HYPERS[0], dict(lr=3e-4, weight_decay=1e-3), GROUP_HYPERS[1]]      # the middle one stays empty
KINDS = {"adam": (torch.optim.Adam, {}), "adamw": (torch.optim.AdamW, {}),
         "sgd": (torch.optim.SGD, dict(momentum=0.9, nesterov=False)),
         "sgd_nesterov": (torch.optim.SGD, dict(momentum=0.9, nesterov=True))}
STATE_KEYS = {"adam": ("exp_avg", "exp_avg_sq"), "adamw": ("exp_avg", "exp_avg_sq"), "sgd": ("momentum_buffer",),
              "sgd_nesterov": ("momentum_buffer",)}


def make_grads(shapes, steps=STEPS, seed=0):
    """grads[step][i]: N(0,1) * 10^U(-10,0) per element, 5 % exact zeros (f32)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        row = []
        for s in shapes:
            x = torch.randn(s, generator=g, dtype=torch.float64) * 10.0 ** (-10.0 * torch.rand(s, generator=g, dtype=torch.float64))
            x[torch.rand(s, generator=g) < 0.05] = 0.0
            row.append(x.float())
        out.append(row)
    return out


def make_params(shapes, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [(0.05 * torch.randn(s, generator=g)).float() for s in shapes]


def build_optimizer(kind, params, membership, hypers=None):
    """torch optimizer of ``kind`` over ``params`` (list of Parameters); ``membership[i]`` = group of params[i] or None (in no
    group).  Groups that end up empty stay in ``param_groups`` (build_optimizer of the harness produces such groups too)."""
    cls, extra = KINDS[kind]
    hypers = hypers or GROUP_HYPERS
    n_groups = max(m for m in membership if m is not None) + 1
    groups = [dict(params=[p for p, m in zip(params, membership) if m == k], **hypers[k]) for k in range(n_groups)]
    return cls(groups, lr=1e-3, foreach=False, **extra)


class Shadow:
    """torch's own optimizer of ``kind`` on CPU copies of ``params0`` in ``dtype``, stepped on gradients handed to it; parameters
    listed in ``no_grad`` keep ``.grad = None``."""

    def __init__(self, kind, params0, membership, dtype, no_grad=(), hypers=None):
        self.kind, self.dtype, self.no_grad = kind, dtype, set(no_grad)
        self.params = [torch.nn.Parameter(p.to(dtype).clone()) for p in params0]
        self.opt = build_optimizer(kind, self.params, membership, hypers)

    def step(self, row, grad_scale=1.0):
        for i, (p, g) in enumerate(zip(self.params, row)):
            p.grad = None if i in self.no_grad else (g.to(self.dtype) * grad_scale)
        self.opt.step()

    def result(self):
        st = self.opt.state
        state = {k: [st[p][k].detach().clone() if p in st and st[p].get(k) is not None else None for p in self.params]
                 for k in STATE_KEYS[self.kind]}
        return [p.detach().clone() for p in self.params], state


def run_reference(kind, params0, grads, membership, dtype, no_grad=(), hypers=None, grad_scale=1.0):
    """(final parameters, {state key: [tensor or None per parameter]}) of torch's own optimizer in ``dtype``."""
    sh = Shadow(kind, params0, membership, dtype, no_grad, hypers)
    for row in grads:
        sh.step(row, grad_scale)
    return sh.result()


def gate(name, got, ref32, ref64, report=None):
    """dev_engine <= 4 * dev_torch; exact equality where dev_torch is 0.  Prints the figures before asserting."""
    dev_torch = float((ref32.double() - ref64).abs().max()) if ref32.numel() else 0.0
    dev_engine = float((got.double() - ref64).abs().max()) if got.numel() else 0.0
    line = f"{name}: dev_engine {dev_engine:.3e} dev_torch {dev_torch:.3e} ratio {dev_engine / dev_torch if dev_torch else float('nan'):.3f}"
    print(line)
    if report is not None:
        report.append(line)
    if dev_torch == 0.0:
        assert torch.equal(got.float(), ref32.float()), line
    else:
        assert dev_engine <= GATE * dev_torch, line


def kernel_restatement(kind, params0, grads, membership, hypers=None, variant=None, grad_scale=1.0):
    """The arithmetic of csrc/optim.hip's Adam kinds restated with f32 torch ops in the kernel's operation order (host scalars in
    double, rounded once).  ``variant="eps_in_sqrt"``: a deliberately wrong denominator, sqrt(v / bc2 + eps)."""
    hypers = hypers or GROUP_HYPERS
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    ps = [p.clone() for p in params0]
    ms = [torch.zeros_like(p) for p in params0]
    vs = [torch.zeros_like(p) for p in params0]
    b1, b2, eps = 0.9, 0.999, 1e-8
    for t, row in enumerate(grads, 1):
        for i, g in enumerate(row):
            if membership[i] is None:
                continue
            h = hypers[membership[i]]
            lr, wd = h["lr"], h["weight_decay"]
            g = g * f(grad_scale)
            if kind == "adam":
                g = g + f(wd) * ps[i]
            else:
                ps[i] = ps[i] * f(1.0 - lr * wd)
            ms[i] = ms[i] + (g - ms[i]) * f(1.0 - b1)
            vs[i] = vs[i] * f(b2) + f(1.0 - b2) * g * g
            sbc2 = f((1.0 - b2 ** t) ** 0.5)
            if variant == "eps_in_sqrt":
                denom = (vs[i] / (sbc2 * sbc2) + f(eps)).sqrt()
            else:
                denom = vs[i].sqrt() / sbc2 + f(eps)
            ps[i] = ps[i] - f(lr / (1.0 - b1 ** t)) * ms[i] / denom
    return ps, {"exp_avg": ms, "exp_avg_sq": vs}
