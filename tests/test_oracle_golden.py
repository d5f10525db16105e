"""Pin the CPU oracle (oracle/ref_cpu.py) against tensors produced by the
reference's own model files (tests/golden/*.npz, written by make_golden.py)."""
import json
import os

import pytest
import torch

from conftest import GOLDEN, golden_param_dict, load_golden, max_rel, rel_err
from oracle import ref_cpu

CASES = ["tiny_kadaptation", "tiny_lora", "tiny_lora_r8", "tiny_adapter", "tiny_compacter"]
TOL = 2e-5   # fp32 CPU vs fp32 CPU, different op order only in reductions
# Gradients that are sums with heavy cancellation (e.g. adapter_up.bias at B=4) carry fp32
# noise of ~3e-4 in the *reference* itself (measured against an fp64 run of this oracle:
# reference 2.7e-4, oracle 8e-5), so the gradient gate is 1e-3 relative-L2.
GTOL = 1e-3


def make_trainer(meta, tensors):
    p = golden_param_dict(meta, tensors)
    tr = ref_cpu.OracleTrainer(p, meta["method"], meta["classes"], lr=meta["lr"], wd=meta["wd"])
    with torch.no_grad():
        tr.head_w.copy_(tensors["head_w"]); tr.head_b.copy_(tensors["head_b"])
    return tr


@pytest.mark.parametrize("case", CASES)
def test_forward_and_grads_match_reference(case):
    meta, t = load_golden(case)
    tr = make_trainer(meta, t)
    feat = ref_cpu.visual_forward(t["images"], tr.p, meta["method"]).detach()
    assert max_rel(feat, t["feat"]) < TOL
    logits, loss = tr.loss_and_grads(t["images"], t["labels"])
    assert max_rel(logits, t["logits0"]) < TOL
    assert abs(float(loss) - float(t["loss0"])) < 1e-5
    none = {n[len("backbone."):] for n in meta["grad_is_none"]}
    checked = 0
    for name in tr.names:
        g = tr.p[name].grad
        if name in none:
            assert g is None, name
            continue
        ref = t["grad/backbone." + name]
        assert rel_err(g, ref) < GTOL, (name, rel_err(g, ref))
        checked += 1
    assert rel_err(tr.head_w.grad, t["grad/layers.0.weight"]) < GTOL
    assert rel_err(tr.head_b.grad, t["grad/layers.0.bias"]) < GTOL
    assert checked > 0


@pytest.mark.parametrize("case", CASES)
def test_sgd_trajectory_matches_reference(case):
    meta, t = load_golden(case)
    tr = make_trainer(meta, t)
    losses = []
    for _ in range(meta["steps"]):
        _, loss = tr.step(t["images"], t["labels"])
        losses.append(float(loss))
    for a, b in zip(losses, meta["losses"]):
        assert abs(a - b) < 2e-4 * max(1.0, abs(b)), (losses, meta["losses"])
    for name in tr.names:
        assert rel_err(tr.p[name].detach(), t["final/backbone." + name]) < 2e-4, name
    assert rel_err(tr.head_w.detach(), t["final/layers.0.weight"]) < 2e-4
    assert rel_err(tr.bn.running_mean, t["bn_mean"]) < 1e-4
    assert rel_err(tr.bn.running_var, t["bn_var"]) < 1e-4


@pytest.mark.parametrize("case", CASES)
def test_trainable_inventory_matches_reference(case):
    meta, t = load_golden(case)
    p = golden_param_dict(meta, t)
    names = ref_cpu.trainable_names(p, meta["method"])
    assert sorted(names) == sorted(meta["trainable_names"])
    n_adapter = sum(p[k].numel() for k in names)
    assert n_adapter == meta["n_adapter_params"]           # bit-exact count
    shapes = ref_cpu.adapter_param_shapes(meta["method"], 128, 2, meta["lora_r"])
    trainable_shapes = {k: v for k, v in shapes.items() if ref_cpu.is_trainable(meta["method"], k)}
    assert {k: tuple(p[k].shape) for k in names} == trainable_shapes


def test_reference_init_values():
    """Degenerate init of the Kronecker factors is what the fixture holds."""
    meta, t = load_golden("tiny_kadaptation")
    for k, v in t.items():
        if k.startswith("init/") and ("adapter1" in k or k.endswith("attn.b")):
            assert float(v.abs().max()) == 0.0, k
        if k.startswith("init/") and "phm_rule" in k:
            assert 0 < float(v.abs().max()) <= 0.01


def test_published_param_counts():
    """README.md:84-87 counts = adapter params + 29,523 (mean head); the adapter part is exact."""
    with open(os.path.join(GOLDEN, "param_counts.json")) as f:
        table = json.load(f)
    expect = {"kadaptation": 50176, "lora": 147456, "adapter": 1208064, "compacter": 48384}
    for m, n in expect.items():
        assert table[f"ViT-B/32|{m}"]["n_adapter"] == n
        assert table[f"ViT-B/16|{m}"]["n_adapter"] == n
        shapes = ref_cpu.adapter_param_shapes(m, 768, 12)
        total = sum(int(torch.Size(s).numel()) for s in shapes.values())
        if m == "compacter":
            total -= 64           # phm_rule (4,4,4) is frozen: name lacks 'compacter'
        assert total == n
    assert table["ViT-L/14|kadaptation"]["n_adapter"] == 126976
    assert table["ViT-L/14|lora"]["n_adapter"] == 393216
    assert table["ViT-L/14|adapter"]["n_adapter"] == 3220992
    assert table["ViT-L/14|compacter"]["n_adapter"] == 127488
    assert table["ViT-B/32|kadaptation|full"]["n_backbone"] == 151327489
    assert 50176 + 29523 == 79699 and 147456 + 29523 == 176979
    assert 1208064 + 29523 == 1237587 and 48384 + 29523 == 77907


def test_rank_r_identity():
    """sum_i kron(s_i t_i^T, l_i r_i^T) == P Q^T   -- the identity the HIP
    path relies on to never materialise H."""
    g = torch.Generator().manual_seed(0)
    n, f = 32, 24
    s = torch.randn(n, n, 1, generator=g); tt = torch.randn(n, 1, n, generator=g)
    l = torch.randn(n, f, 1, generator=g); r = torch.randn(n, 1, f, generator=g)
    H = ref_cpu.kron_sum(torch.bmm(s, tt), torch.bmm(l, r))
    P = torch.stack([torch.kron(s[i, :, 0], l[i, :, 0]) for i in range(n)], dim=1)
    Q = torch.stack([torch.kron(tt[i, 0], r[i, 0]) for i in range(n)], dim=1)
    assert max_rel(P @ Q.T, H) < 1e-5


FULL = ["full_b32_kadaptation", "full_b32_lora", "full_b32_adapter", "full_b32_compacter",
        # the architectures of BASELINE configs 3-5 (LoRA r=8; ViT-B/16 + Compacter; ViT-L/14 + KAdaptation)
        "full_b32_lora_r8", "full_b16_compacter", "full_l14_kadaptation"]


@pytest.mark.parametrize("case", FULL)
def test_full_size_vit_matches_reference(case):
    """Full width / depth, bs=8, C=100: logits / loss / per-tensor gradient norms recorded from the
    reference.  The 88-304M-parameter state-dict is regenerated from its seed (checksummed)."""
    from pevit_amd.synth import ARCHS, randomize_adapters, synth_batch, synth_state_dict
    meta, t = load_golden(case)
    method = meta["method"]
    arch = ARCHS[meta["arch"]]
    sd = synth_state_dict(arch, seed=2, text_tower=False)
    for k, (s1, s2) in meta["sd_checksum"].items():
        assert abs(float(sd[k].double().sum()) - s1) <= 1e-6 * max(1.0, abs(s1)), "generator drift: " + k
        assert abs(float((sd[k].double() ** 2).sum()) - s2) <= 1e-6 * max(1.0, abs(s2)), "generator drift: " + k
    p = {k: v for k, v in sd.items() if k.startswith("visual.")}
    shapes = ref_cpu.adapter_param_shapes(method, arch.width, arch.layers, meta["lora_r"])
    ordered = [(n, torch.zeros(shapes[n])) for n in meta["trainable_names"]]
    randomize_adapters(ordered, seed=3)
    p.update(dict(ordered))
    for k, v in t.items():
        if k.startswith("adapter/"):
            p[k[len("adapter/"):]] = v.float()
    tr = ref_cpu.OracleTrainer(p, method, meta["classes"], lr=meta["lr"], wd=meta["wd"])
    images, labels = synth_batch(meta["batch"], arch.resolution, meta["classes"])
    logits, loss = tr.loss_and_grads(images, labels)
    assert max_rel(logits, t["logits0"]) < 1e-4
    assert abs(float(loss) - float(t["loss0"])) < 1e-4
    none = set(meta["grad_is_none"])
    for name in tr.names:
        ref = meta["grad_norms"]["backbone." + name]
        if ("backbone." + name) in none:
            assert tr.p[name].grad is None
        else:
            got = float(tr.p[name].grad.double().norm())
            assert abs(got - ref) <= 2e-3 * max(ref, 1e-6), (name, got, ref)
            # ... and the 32 recorded sign projections of the tensor (round 5): a norm cannot see a permutation or a sign
            k = "backbone." + name
            if "grad_proj/" + k in t:
                from conftest import proj_rel_err
                e = proj_rel_err(tr.p[name].grad, meta["proj_index"][k], t["grad_proj/" + k], ref)
                assert e < 5e-3, (name, e)
    assert tr.n_trainable() == meta["n_trainable_params"]


REFINIT = ["full_b32_kadaptation_refinit", "full_b32_lora_r8_refinit", "full_b32_adapter_refinit"]


@pytest.mark.parametrize("case", REFINIT)
def test_oracle_trajectory_at_reference_init(case):
    """The oracle against the *_refinit fixtures (full width / depth, bs 8, the reference's own initialisation, five SGD steps):
    logits / loss of step 0, every recorded gradient of the first and of the LAST step, what the steps changed, the loss
    trajectory.  (ViT-B/16 Compacter and ViT-L/14 have the same fixtures; they are compared on the GPU only -- tests/test_gpu_refinit.py
    -- to keep this suite at minutes.)"""
    from conftest import proj_rel_err
    from pevit_amd.synth import ARCHS, reference_init_, synth_batch, synth_state_dict
    meta, t = load_golden(case)
    method, arch = meta["method"], ARCHS[meta["arch"]]
    sd = synth_state_dict(arch, seed=2, text_tower=False)
    p = {k: v for k, v in sd.items() if k.startswith("visual.")}
    shapes = ref_cpu.adapter_param_shapes(method, arch.width, arch.layers, meta["lora_r"])
    named = [(n, torch.zeros(shapes[n])) for n in meta["trainable_names"]]
    if "init_checksum" in meta:
        reference_init_(named, method, seed=7)
    p.update(dict(named))
    for k, v in t.items():
        if k.startswith("adapter/"):
            p[k[len("adapter/"):]] = v.float().view(shapes[k[len("adapter/"):]])
    tr = ref_cpu.OracleTrainer(p, method, meta["classes"], lr=meta["lr"], wd=meta["wd"])
    with torch.no_grad():
        tr.head_w.copy_(t["head_w"]); tr.head_b.copy_(t["head_b"])
    init = {n: tr.p[n].detach().clone() for n in tr.names}
    init["layers.0.weight"], init["layers.0.bias"] = tr.head_w.detach().clone(), tr.head_b.detach().clone()
    images, labels = synth_batch(meta["batch"], arch.resolution, meta["classes"])

    def check(kind, key, v, tol):
        if f"{kind}/{key}" in t:
            e = rel_err(v, t[f"{kind}/{key}"].view_as(v))
            assert e < tol, (kind, key, e)
            return 1
        if f"{kind}_proj/{key}" in t:
            e = proj_rel_err(v, meta["proj_index"][key], t[f"{kind}_proj/{key}"], t[f"{kind}_norm/{key}"])
            assert e < tol, (kind, key, e)
            return 1
        assert v is None or float(v.abs().max()) == 0.0, (kind, key)        # the reference left it exactly zero / untouched
        return 0

    losses = []
    for step in range(meta["steps"]):
        logits, loss = tr.loss_and_grads(images, labels)
        losses.append(float(loss))
        if step == 0:
            assert max_rel(logits, t["logits0"]) < 1e-4 and abs(float(loss) - float(t["loss0"])) < 1e-4
        if step in (0, meta["steps"] - 1):
            kind = "grad" if step == 0 else "grad_last"
            n = sum(check(kind, "backbone." + name, tr.p[name].grad, 5e-3) for name in tr.names)
            n += check(kind, "layers.0.weight", tr.head_w.grad, 5e-3) + check(kind, "layers.0.bias", tr.head_b.grad, 5e-3)
            assert n == sum(k.startswith((kind + "/", kind + "_proj/")) for k in t)
        tr.opt.step()
    for a, b in zip(losses, meta["losses"]):
        assert abs(a - b) < 1e-3 * max(1.0, abs(b)), (losses, meta["losses"])
    n = sum(check("delta", "backbone." + name, tr.p[name].detach() - init[name], 5e-3) for name in tr.names)
    n += check("delta", "layers.0.weight", tr.head_w.detach() - init["layers.0.weight"], 5e-3)
    n += check("delta", "layers.0.bias", tr.head_b.detach() - init["layers.0.bias"], 5e-3)
    assert n == sum(k.startswith(("delta/", "delta_proj/")) for k in t)


ALL_REFINIT = REFINIT + ["full_b16_compacter_refinit", "full_l14_kadaptation_refinit"]


@pytest.mark.parametrize("case", ALL_REFINIT)
def test_refinit_fixtures_carry_the_reference_recorded_bf16_floor(case):
    """Round 6: every *_refinit fixture holds, next to the reference's f32 results, how far the REFERENCE ITSELF moves when its frozen
    weights (leg "weights") and all its contraction operands (leg "operands"; ViT-L/14 also "fp8") are rounded to bf16
    (tests/golden/make_golden.py --refinit --bf16-weights).  tests/test_gpu_refinit.py gates the production kernels at
    max(stated gate, FLOOR_C x this floor) with FLOOR_C = 3; here: the floor is complete (an entry for every recorded tensor), finite, and the weights-only
    leg keeps the logits within the stated 2e-2 on every fixture -- i.e. bf16 WEIGHTS alone never cost a stated gate on the logits."""
    import math
    meta, t = load_golden(case)
    fl = meta["floor"]
    legs = ["weights", "operands"] + (["fp8"] if "l14" in case else [])
    for leg in legs:
        d = fl[leg]
        for kind in ("grad", "grad_last", "delta"):
            recorded = {k.split("/", 1)[1] for k in t if k.startswith((kind + "/", kind + "_proj/"))}
            assert recorded <= set(d[kind]), (leg, kind, sorted(recorded - set(d[kind]))[:3])
            assert all(math.isfinite(v) and v >= 0.0 for v in d[kind].values())
            assert math.isfinite(d[kind + "_all"]) and 0.0 <= d[kind + "_all"] < 1.0
        assert len(d["loss_traj"]) == meta["steps"] and all(math.isfinite(v) for v in d["loss_traj"])
    assert fl["weights"]["logits"] < 2e-2
    # the operand leg contains the weight leg's rounding: on the whole step it is not smaller (up to the noise of two draws)
    assert fl["operands"]["grad_all"] > 0.5 * fl["weights"]["grad_all"]
