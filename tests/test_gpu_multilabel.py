"""Multi-label fine-tuning on the GPU: the head with BCEWithLogitsLoss (bce_loss_kernel) against torch f32, the engine's target
forms, the fused BCE step against the autograd route and against the f32 oracle, its uint8 / graph / two-rank forms, and one CLI
run on a multi-hot archive (the reference trains voc-2007-classification and chestx-ray8 this way, kadaptation_clip.py:273-276)."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from conftest import ROOT, golden_param_dict, load_golden, load_tiny_sd, max_rel, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def multi_hot(B, C, seed, p=0.2):
    g = torch.Generator().manual_seed(seed)
    y = (torch.rand(B, C, generator=g) < p).float()
    y[torch.arange(B), torch.randint(0, C, (B,), generator=g)] = 1.0
    return y


def _engine(B, C, method="kadaptation", arch="tiny-128"):
    from pevit_amd.engine import HipEngine
    from pevit_amd.synth import ARCHS
    return HipEngine(ARCHS[arch], method, C, B)


# ------------------------------------------------------------------------------------------------ head + BCE vs torch f32
@pytest.mark.parametrize("kind", ["multi_hot", "soft", "wide"])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("B,C", [(7, 3), (16, 10), (128, 20), (128, 130), (2050, 14)])
def test_head_batchnorm_linear_bce(B, C, training, kind):
    """BatchNorm1d -> Linear -> BCEWithLogitsLoss(mean), forward and backward, at the gates of the cross-entropy head test.
    "wide" scales the head so that the logits reach +-60; "soft" uses targets in [0, 1]."""
    eng = _engine(B, C)
    D = eng.arch.embed_dim
    feat = rnd(B, D, seed=1, scale=1.5) + 0.3
    W = rnd(C, D, seed=3, scale=0.2); bias = rnd(C, seed=4, scale=0.2)
    rm0 = rnd(D, seed=5, scale=0.1); rv0 = rnd(D, seed=6, scale=0.1).abs() + 0.5
    if kind == "wide":                                          # the largest logit magnitude becomes 58 (+ its bias)
        z = F.batch_norm(feat, rm0.clone(), rv0.clone(), None, None, training, 0.1, 1e-5) @ W.t()
        W = W * (58.0 / float(z.abs().max()))
    if kind == "soft":
        targets = torch.rand(B, C, generator=torch.Generator().manual_seed(2)).cuda()
    else:
        targets = multi_hot(B, C, seed=2).cuda()
    v = eng.param_views()
    with torch.no_grad():
        v["layers.0.weight"].copy_(W); v["layers.0.bias"].copy_(bias)
    runs = []
    for _ in range(2):
        eng.running_mean.copy_(rm0); eng.running_var.copy_(rv0)
        eng.zero_grad()
        logits, loss, dfeat = eng.head_forward_backward(feat, targets, bn_training=training)
        torch.cuda.synchronize()
        gv = eng.grad_views()
        runs.append([t.clone() for t in (logits, loss, dfeat, gv["layers.0.weight"], gv["layers.0.bias"], eng.running_mean,
                                          eng.running_var)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)                               # the same bits on every call
    logits, loss, dfeat, gW, gb, rm_out, rv_out = runs[0]
    f = feat.clone().requires_grad_(True); Wr = W.clone().requires_grad_(True); br = bias.clone().requires_grad_(True)
    rm, rv = rm0.clone(), rv0.clone()
    ref_logits = F.linear(F.batch_norm(f, rm, rv, None, None, training, 0.1, 1e-5), Wr, br)
    ref_loss = F.binary_cross_entropy_with_logits(ref_logits, targets)
    ref_loss.backward()
    if kind == "wide":
        assert float(ref_logits.detach().abs().max()) > 55.0
    assert max_rel(logits.cpu(), ref_logits.detach().cpu()) < 1e-5
    assert abs(float(loss) - float(ref_loss.detach())) < 1e-5, (float(loss), float(ref_loss.detach()))
    assert max_rel(dfeat.cpu(), f.grad.cpu()) < 2e-5
    assert max_rel(gW.cpu(), Wr.grad.cpu()) < 2e-5
    assert max_rel(gb.cpu(), br.grad.cpu()) < 2e-5
    assert max_rel(rm_out.cpu(), rm.cpu()) < 1e-6 and max_rel(rv_out.cpu(), rv.cpu()) < 1e-6
    assert torch.isfinite(loss).all() and torch.isfinite(dfeat).all()


# ------------------------------------------------------------------------------------------------ the engine's target forms
def test_engine_takes_multi_hot_targets_and_refuses_the_rest():
    from pevit_amd import _lib
    B, C = 4, 10
    eng = _engine(B, C, method="lora")
    img = torch.randn(B, 3, 48, 48).cuda()
    y = multi_hot(B, C, seed=1).cuda()
    logits, loss = eng.forward_backward(img, y)
    ref = F.binary_cross_entropy_with_logits(logits.float(), y)
    assert abs(float(loss) - float(ref)) < 1e-5
    lab = torch.tensor([1, 0, 3, 9]).cuda()                  # int64 (B,) still selects cross-entropy
    logits, loss = eng.forward_backward(img, lab)
    assert abs(float(loss) - float(F.cross_entropy(logits.float(), lab))) < 1e-5
    bad = (y.double(), y[:, 0].contiguous(), y.cpu(), torch.zeros(B, C + 1).cuda(), y.t().contiguous().t(), y.long(),
           y[:3].contiguous(), torch.zeros(B, 1).cuda())
    for t in bad:
        with pytest.raises(_lib.PevitError):
            eng.forward_backward(img, t)
        with pytest.raises(_lib.PevitError):
            eng.head_forward_backward(torch.randn(B, eng.arch.embed_dim).cuda(), t)
    eng.train_step(img, y, lr=0.01)
    for t in bad[:4]:
        with pytest.raises(_lib.PevitError):
            eng.capture_train_step(img, t, lr=0.01)
        with pytest.raises(_lib.PevitError):
            eng.forward_backward_dp(img, t, mode="staged")


# ------------------------------------------------------------------------------------------------ fused route vs autograd route
class MultiHotBatch:
    """A loader that yields one batch ``steps`` times with (B, C) float targets."""

    def __init__(self, images, targets, steps):
        self.batch, self.steps = (images, targets), steps
        self.dataset = range(images.shape[0] * steps)

    def __iter__(self):
        return iter([self.batch] * self.steps)


def _targets_of(t, classes, seed=0):
    """multi-hot targets from a fixture's class labels: its class plus a second one per row"""
    y = F.one_hot(t["labels"], classes).float()
    y[torch.arange(len(y)), (t["labels"] + 1 + seed) % classes] = 1.0
    return y


@pytest.mark.parametrize("method,nesterov", [("kadaptation", False), ("compacter", False), ("lora", True)])
def test_fused_and_autograd_bce_routes_agree(method, nesterov, tmp_path):
    from test_gpu_mirror import seeded_classifier
    ckpt = tmp_path / "tiny.pt"
    torch.save(load_tiny_sd(), ckpt)
    meta, t = load_golden("tiny_" + method)
    y = _targets_of(t, meta["classes"])
    outs, calls = {}, {}
    for route in ("fused", "autograd"):
        mod, cfg, clf = seeded_classifier(method, ckpt, meta, t, NESTEROV=nesterov)
        opt = mod.build_optimizer(cfg, clf)
        crit = torch.nn.BCEWithLogitsLoss().cuda(0)
        if route == "autograd":
            clf.can_fuse = lambda *_: False
        else:
            assert clf.can_fuse(crit, opt)
        n = [0]
        step = clf.fused_train_step

        def counted(*a, **k):
            n[0] += 1
            return step(*a, **k)
        clf.fused_train_step = counted
        mod.train_one(MultiHotBatch(t["images"], y, 2), clf, crit, opt, 0, cfg)
        calls[route] = n[0]
        outs[route] = {n_: p.detach().cpu().clone() for n_, p in clf.named_parameters() if p.requires_grad}
        outs[route]["bn_mean"] = clf.channel_bn.running_mean.cpu().clone()
        del clf, opt
    assert calls == {"fused": 2, "autograd": 0}
    for n_, a in outs["fused"].items():
        assert rel_err(a, outs["autograd"][n_]) < 5e-3, (n_, rel_err(a, outs["autograd"][n_]))


# ------------------------------------------------------------------------------------------------ fused step vs the f32 oracle
def _bce_oracle():
    from oracle import ref_cpu

    class BceOracle(ref_cpu.OracleTrainer):
        def loss_and_grads(self, images, targets):
            self.opt.zero_grad(set_to_none=True)
            logits = self.forward(images)
            loss = F.binary_cross_entropy_with_logits(logits, targets)
            loss.backward()
            return logits.detach(), loss.detach()
    return BceOracle


@pytest.mark.parametrize("case", ["tiny_kadaptation", "tiny_lora", "tiny_adapter", "tiny_compacter"])
def test_bce_step_error_is_bf16_operand_rounding(case):
    from oracle import ref_cpu
    from test_gpu_tower import make_engine
    meta, t = load_golden(case)
    eng, sd = make_engine(meta, t)
    y = _targets_of(t, meta["classes"])
    Oracle = _bce_oracle()

    def run(emulate):
        tr = Oracle(sd, meta["method"], meta["classes"])
        with torch.no_grad():
            tr.head_w.copy_(t["head_w"]); tr.head_b.copy_(t["head_b"])
        if emulate:
            with ref_cpu.operand_rounding(torch.bfloat16):
                lg, ls = tr.loss_and_grads(t["images"], y)
        else:
            lg, ls = tr.loss_and_grads(t["images"], y)
        return tr, lg, ls
    f32, l32, loss32 = run(False)
    emu, lemu, _ = run(True)
    logits, loss = eng.forward_backward(t["images"].cuda(), y.cuda())
    torch.cuda.synchronize()
    assert max_rel(logits.cpu(), l32) <= 2.5 * max_rel(lemu, l32) + 5e-3
    assert abs(float(loss) - float(loss32)) < 2e-2
    gv = eng.grad_views()
    hip_w = max(rel_err(gv[n].cpu(), f32.p[n].grad) for n in f32.names if f32.p[n].grad is not None)
    emu_w = max(rel_err(emu.p[n].grad, f32.p[n].grad) for n in f32.names if f32.p[n].grad is not None)
    assert hip_w <= 2.5 * emu_w + 1e-2, (hip_w, emu_w)
    for w in ("layers.0.weight", "layers.0.bias"):
        g_ref = f32.head_w.grad if w.endswith("weight") else f32.head_b.grad
        assert rel_err(gv[w].cpu(), g_ref) <= 2.5 * emu_w + 1e-2


# ------------------------------------------------------------------------------------------------ uint8 pixels, graph replay
def _synth_engines(n, B, C, method="kadaptation"):
    from pevit_amd.engine import HipEngine, adapter_param_spec
    from pevit_amd.synth import ARCHS, randomize_adapters, synth_state_dict
    arch = ARCHS["tiny-128"]
    sd = {k: v for k, v in synth_state_dict(arch, seed=2, text_tower=False).items() if k.startswith("visual.")}
    ad = [(nm, torch.zeros(s)) for nm, s, _ in adapter_param_spec(method, arch.width, arch.layers)]
    randomize_adapters(ad, seed=3); sd.update(dict(ad))
    engs = []
    for _ in range(n):
        e = HipEngine(arch, method, C, B)
        e.load_state_dict(sd)
        torch.nn.init.normal_(e.param_views()["layers.0.weight"], std=0.05, generator=torch.Generator(device="cuda").manual_seed(1))
        engs.append(e)
    return arch, engs


def test_uint8_pixels_give_the_bits_of_host_normalised_f32():
    B, C = 8, 20
    arch, (eu, ef) = _synth_engines(2, B, C)
    mean, std = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
    eu.set_input_normalization(mean, std)
    g = torch.Generator().manual_seed(7)
    u8 = torch.randint(0, 256, (B, 3, arch.resolution, arch.resolution), generator=g, dtype=torch.uint8)
    f32 = (u8.float() / 255.0 - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1)
    y = multi_hot(B, C, seed=8).cuda()
    for step in range(2):
        l0, s0 = eu.train_step(u8.cuda(), y, lr=0.05, momentum=0.9, weight_decay=1e-4)
        l1, s1 = ef.train_step(f32.contiguous().cuda(), y, lr=0.05, momentum=0.9, weight_decay=1e-4)
        torch.cuda.synchronize()
        assert torch.equal(l0, l1) and torch.equal(s0, s1), step
        assert torch.equal(eu.params, ef.params) and torch.equal(eu.grads, ef.grads), step


def test_bce_graph_replay_equals_eager():
    B, C = 8, 20
    arch, (eager, graphed) = _synth_engines(2, B, C)
    from pevit_amd.synth import synth_batch
    images, _ = synth_batch(B, arch.resolution, C)
    images, y = images.cuda(), multi_hot(B, C, seed=9).cuda()
    graphed.params.copy_(eager.params)
    for e in (eager, graphed):
        e.train_step(images, y, lr=0.05, momentum=0.9, weight_decay=1e-4)
    replay = graphed.capture_train_step(images, y, lr=0.05, momentum=0.9, weight_decay=1e-4)
    for step in range(4):
        l0, s0 = eager.train_step(images, y, lr=0.05, momentum=0.9, weight_decay=1e-4)
        l1, s1 = replay()
        torch.cuda.synchronize()
        assert torch.equal(l0, l1) and torch.equal(s0, s1), step
        for a, b in ((eager.params, graphed.params), (eager.momentum, graphed.momentum), (eager.grads, graphed.grads),
                     (eager.running_mean, graphed.running_mean), (eager.running_var, graphed.running_var)):
            assert torch.equal(a, b), step


# ------------------------------------------------------------------------------------------------ two ranks on one GPU
DP_STEPS, LR, MOM, WD = 3, 0.05, 0.9, 1e-3


def _dp_engine(case, batch):
    from pevit_amd.engine import HipEngine
    from pevit_amd.synth import ARCHS
    meta, t = load_golden(case)
    eng = HipEngine(ARCHS[meta["arch"]], meta["method"], meta["classes"], batch, lora_rank=meta["lora_r"])
    eng.load_state_dict(golden_param_dict(meta, t))
    v = eng.param_views()
    with torch.no_grad():
        v["layers.0.weight"].copy_(t["head_w"]); v["layers.0.bias"].copy_(t["head_b"])
    return eng, meta, t


def _dp_shard(meta, t, rank, world):
    img = torch.cat([t["images"], t["images"].flip(0) * 0.5])
    y = torch.cat([_targets_of(t, meta["classes"]), _targets_of(t, meta["classes"], seed=1).flip(0)])
    n = img.shape[0] // world
    return img[rank * n:(rank + 1) * n].cuda().contiguous(), y[rank * n:(rank + 1) * n].cuda().contiguous()


def _dp_worker(rank, world, port, case, out_dir, mode):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng, meta, t = _dp_engine(case, 4)
    eng.dp_exchange_mode = mode
    eng.sync_replicas()
    img, y = _dp_shard(meta, t, rank, world)
    losses = []
    for _ in range(DP_STEPS):
        _, loss = eng.train_step(img, y, lr=LR, momentum=MOM, weight_decay=WD, world_size=world)
        losses.append(float(loss))
    torch.cuda.synchronize()
    torch.save({"p": eng.params.cpu(), "m": eng.momentum.cpu(), "losses": losses}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["single", "staged"])
def test_two_rank_bce_step_equals_mean_of_shard_steps(mode, tmp_path):
    case, world = "tiny_kadaptation", 2
    port = 31700 + (os.getpid() % 2000) + {"single": 0, "staged": 11}[mode]
    mp.spawn(_dp_worker, args=(world, port, case, str(tmp_path), mode), nprocs=world, join=True)
    r0 = torch.load(tmp_path / "rank0.pt"); r1 = torch.load(tmp_path / "rank1.pt")
    assert torch.equal(r0["p"], r1["p"]) and torch.equal(r0["m"], r1["m"])
    e0, meta, t = _dp_engine(case, 4); e1, _, _ = _dp_engine(case, 4)
    shards = [_dp_shard(meta, t, r, world) for r in range(world)]
    for step in range(DP_STEPS):
        l0 = float(e0.forward_backward(*shards[0])[1]); l1 = float(e1.forward_backward(*shards[1])[1])
        assert l0 == r0["losses"][step] and l1 == r1["losses"][step]
        total = e0.grads + e1.grads
        for e in (e0, e1):
            e.grads.copy_(total)
            e.sgd_step(LR, MOM, WD, 1.0 / world)
    torch.cuda.synchronize()
    assert torch.equal(e0.params.cpu(), r0["p"]) and torch.equal(e0.momentum.cpu(), r0["m"])


# ------------------------------------------------------------------------------------------------ the CLI on a multi-hot archive
def test_kadaptation_command_on_a_multi_hot_archive(tmp_path, monkeypatch):
    from pevit_amd.commands import _finetune
    from pevit_amd.commands import kronecker_adaptation_clip as cmd
    from pevit_amd.config import default_config
    from pevit_amd.evaluation import _harness
    ckpt = tmp_path / "tiny.pt"
    torch.save(load_tiny_sd(), ckpt)
    rng = np.random.default_rng(0)
    n_train, n_test = 60, 16
    ytr = multi_hot(n_train, 20, seed=11).numpy().astype(np.uint8)
    yte = multi_hot(n_test, 20, seed=12).numpy().astype(np.uint8)
    np.savez(tmp_path / "voc-2007-classification.npz", train_images=rng.integers(0, 256, (n_train, 3, 48, 48), dtype=np.uint8),
             train_labels=ytr, test_images=rng.integers(0, 256, (n_test, 3, 48, 48), dtype=np.uint8), test_labels=yte)
    model = tmp_path / "model.yaml"
    model.write_text(f"MODEL:\n  NAME: '{ckpt}'\n  SPEC:\n    EMBED_DIM: 64\nTRAIN:\n  END_EPOCH: 1\n  EXTRA_FINAL_TRAIN_EPOCH: 0\n"
                     "  NESTEROV: false\n  WD: 0.\n")
    monkeypatch.setattr(_finetune, "config", default_config())
    calls = {"fused": 0, "criterion": 0}
    fused = _harness.ClassifierBase.fused_train_step
    crit_forward = torch.nn.BCEWithLogitsLoss.forward

    def count_fused(self, *a, **k):
        calls["fused"] += 1
        return fused(self, *a, **k)

    def count_crit(self, *a, **k):
        calls["criterion"] += 1
        return crit_forward(self, *a, **k)
    monkeypatch.setattr(_harness.ClassifierBase, "fused_train_step", count_fused)
    monkeypatch.setattr(torch.nn.BCEWithLogitsLoss, "forward", count_crit)
    score, info = cmd.main(["--model", str(model), "--no-tuning", "True", "--lr", "0.01", "--l2", "1e-6",
                            "DATASET.DATASET", "voc-2007-classification", "DATASET.NUM_CLASSES", "20", "TEST.METRIC", "11point_mAP",
                            "DATASET.ROOT", str(tmp_path), "OUTPUT_DIR", str(tmp_path / "out"), "TRAIN.IMAGE_SIZE", "[48, 48]"])
    assert calls["fused"] > 0 and calls["criterion"] == 0      # every training step took the fused BCE route
    assert math.isfinite(score) and 0.0 < score <= 100.0
    j = json.load(open(tmp_path / "out" / "predictions" / "finetuning_full" / "seed0_voc-2007-classification.json"))
    assert np.asarray(j["predictions"][0]).shape == (n_test, 20)
