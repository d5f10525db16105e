"""The linear probe's head on cached feature rows (csrc/probe.hip: pevit_probe_step, pevit_probe_predict) against torch f32 on the
same device, under the gates this project already asserts for the same arithmetic (tests/test_gpu_ops2.py:
test_head_batchnorm_linear_cross_entropy and test_fused_sgd_matches_torch_optim): max_rel 1e-5 for logits and loss, 2e-5 for
gradients, 1e-6 for running statistics and updated parameters.  The momentum buffer after a step is the step's gradient plus
two small terms (momentum * old buffer, weight decay * parameter), so it is held to the gradients' gate.

The parameters' gate is the optimizer's own (test_fused_sgd_matches_torch_optim hands both sides the SAME gradient); here the two
sides' gradients may differ by the gradients' gate, and that difference reaches the parameters multiplied by lr * |g| / |W|.  The
two gates are consistent while that factor stays below 1e-6 / 2e-5 = 0.05, so the steps run at lr = 1e-3 (the reference's default
TRAIN.LR), where an update is about a hundredth of the weights: an error of 1e-4 of the update -- any wrong term of the momentum,
Nesterov, weight-decay or first-step rule is of order 1 -- still misses the gate.

Measured at the named tests' own lr = 0.05 (not asserted; the four shapes, CE and BCE, both scales, batch statistics, Nesterov):
the updated weights are within 7.4e-7 of torch's with weights at the named tests' scale 0.2 and within 9.9e-7 at nn.Linear's scale
(D = 512, C = 100, CE at the CLIP scale; 9.5e-7 at D = 768, C = 211), the bias within 3.0e-7 -- inside 1e-6 with no room to spare, as
the factor above says it must be at lr * |g| / |W| near 0.05.  At lr = 1e-3 the worst updated weight of this file is 1.8e-7."""
import math

import numpy as np

import pytest
import torch
import torch.nn.functional as F

from conftest import max_rel

import optim_gate as og

pytestmark = pytest.mark.gpu

GATE_OUT, GATE_GRAD, GATE_STATE = 1e-5, 2e-5, 1e-6
CLIP_SCALE = math.exp(math.log(1 / 0.07))
LR, MOM, WD = 1e-3, 0.9, 1e-2

_ENGINES = {}


def _engine(D, C, max_batch=128):
    """One frozen-tower engine per head shape (the tower is the smallest legal one; only its embed_dim matters here)."""
    from pevit_amd.engine import HipEngine
    from pevit_amd.synth import VitArch
    key = (D, C, max_batch)
    if key not in _ENGINES:
        _ENGINES[key] = HipEngine(VitArch(f"probe-{D}", 128, 2, 16, 48, D), "none", C, max_batch)
    return _ENGINES[key]


def rnd(*shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def _data(B, D, C, bce, seed=0, rows=None, ignore=False):
    """Cached rows, an index list that is a shuffled selection of them with one row taken twice (never arange: the gather is
    real), and labels indexed like the rows.  A batch of two takes two different rows: the same row twice is a batch of variance
    zero, whose normalised rows and weight gradient are exactly zero on both sides."""
    rows = rows or B + 5
    feats = rnd(rows, D, seed=seed + 1, scale=1.5) + 0.3
    g = torch.Generator().manual_seed(seed + 2)
    idx = torch.randperm(rows, generator=g)[:B].clone()
    if B > 2:
        idx[B // 2] = idx[0]
    assert not torch.equal(idx, torch.arange(B))
    if bce:
        labels = (torch.rand((rows, C), generator=g) < 0.3).float()
    else:
        labels = torch.randint(0, C, (rows,), generator=g)
        if ignore:
            labels[idx[1]] = -100
    return feats, idx.cuda(), labels.cuda()


def _set_state(eng, D, C, seed=0, momentum=False):
    """Head weights N(0, 1/D), the scale torch.nn.Linear initialises at (|w| <= 1/sqrt(D)): the pre-scale logits of normalised
    rows then have unit variance whatever D is, and CLIP's scale puts the largest logit near 60.  (At a fixed 0.2 the D = 512 head
    has logits near 250 at that scale, where one f32 rounding of a logit -- 3e-7 relative, 1e-4 absolute -- moves a softmax
    probability by 1e-4 of itself on EITHER side of the comparison.)"""
    v = eng.param_views()
    with torch.no_grad():
        v["layers.0.weight"].copy_(rnd(C, D, seed=seed + 3, scale=D ** -0.5)); v["layers.0.bias"].copy_(rnd(C, seed=seed + 4, scale=0.2))
        eng.running_mean.copy_(rnd(D, seed=seed + 5, scale=0.1)); eng.running_var.copy_(rnd(D, seed=seed + 6, scale=0.1).abs() + 0.5)
    eng.reset_optimizer()
    eng.grads.zero_()
    if momentum:
        eng.momentum.copy_(rnd(eng.n_params, seed=seed + 7, scale=0.01))
        eng._steps = 1                       # not the first step of the run: the momentum buffer is read


def _state(eng):
    """(W, b, momentum of W, momentum of b, running_mean, running_var), copied out"""
    p, m = eng.param_views(), eng.param_views(eng.momentum)
    return [t.detach().clone() for t in (p["layers.0.weight"], p["layers.0.bias"], m["layers.0.weight"], m["layers.0.bias"],
                                         eng.running_mean, eng.running_var)]


def _torch_step(state, feats, idx, labels, training, s, nesterov, first, update=True):
    """The same step in torch f32 on the device from a copied state: (logits, loss, dW, db, new state)."""
    W, b, mW, mb, rm, rv = [t.clone() for t in state]
    W.requires_grad_(True); b.requires_grad_(True)
    x, y = feats[idx], labels[idx]
    logits = s * F.linear(F.batch_norm(x, rm, rv, None, None, training, 0.1, 1e-5), W, b)
    loss = F.binary_cross_entropy_with_logits(logits, y) if y.dtype == torch.float32 else F.cross_entropy(logits, y)
    loss.backward()
    dW, db = W.grad.clone(), b.grad.clone()
    if update:
        opt = torch.optim.SGD([W, b], lr=LR, momentum=MOM, weight_decay=WD, nesterov=nesterov)
        if not first:
            opt.state[W]["momentum_buffer"] = mW; opt.state[b]["momentum_buffer"] = mb
        opt.step()
        mW, mb = opt.state[W]["momentum_buffer"], opt.state[b]["momentum_buffer"]
    return logits.detach(), loss.detach(), dW, db, [W.detach(), b.detach(), mW, mb, rm, rv]


def _check_step(tag, eng, got_logits, got_loss, ref, updated=True):
    ref_logits, ref_loss, dW, db, new = ref
    gv = eng.grad_views()
    figs = {"logits": (max_rel(got_logits, ref_logits), GATE_OUT), "loss": (max_rel(got_loss.view(1), ref_loss.view(1)), GATE_OUT),
            "dW": (max_rel(gv["layers.0.weight"], dW), GATE_GRAD), "db": (max_rel(gv["layers.0.bias"], db), GATE_GRAD)}
    names = ("W", "b", "mom_W", "mom_b", "running_mean", "running_var")
    for n, g, r in zip(names, _state(eng), new):
        if updated or n.startswith("running"):
            figs[n] = (max_rel(g, r), GATE_GRAD if n.startswith("mom") else GATE_STATE)
    print(tag, " ".join(f"{k} {v:.2e}" for k, (v, _) in figs.items()))
    for k, (v, gate) in figs.items():
        assert v <= gate, f"{tag}: {k} max_rel {v:.3e} over the gate {gate:g}"


SHAPES = [(2, 64, 3), (33, 64, 37), (64, 512, 100), (128, 768, 211)]


@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("s", [1.0, CLIP_SCALE], ids=["s1", "sclip"])
@pytest.mark.parametrize("bce", [False, True], ids=["ce", "bce"])
@pytest.mark.parametrize("training", [True, False], ids=["bn_train", "bn_eval"])
@pytest.mark.parametrize("B,D,C", SHAPES)
def test_single_step_matches_torch(B, D, C, training, bce, s, nesterov):
    """One step from a state with a non-zero momentum buffer (not the first step) and non-zero weight decay."""
    eng = _engine(D, C)
    feats, idx, labels = _data(B, D, C, bce)
    _set_state(eng, D, C, momentum=True)
    before = _state(eng)
    logits, loss = eng.probe_step(feats, idx, labels, lr=LR, momentum=MOM, weight_decay=WD, nesterov=nesterov, bn_training=training,
                                  scale=s)
    torch.cuda.synchronize()
    ref = _torch_step(before, feats, idx, labels, training, s, nesterov, first=False)
    _check_step(f"step B{B} D{D} C{C}", eng, logits, loss, ref)


@pytest.mark.parametrize("bce", [False, True], ids=["ce", "bce"])
@pytest.mark.parametrize("B,D,C", [(33, 1024, 300), (64, 1024, 1000)])
def test_step_and_predict_near_the_limits(B, D, C, bce):
    """The widest head the entries accept: D = 1024 is the largest LDS footprint of the forward launch, C = 300 and C = 1000 are
    the two forms with 8 and 16 logit registers per lane (the shapes above stop at 4) and their row grouping of 2 and 1 in the
    loss.  Same gates as every other step; predict runs the same two forms without the loss."""
    eng = _engine(D, C)
    feats, idx, labels = _data(B, D, C, bce, seed=70)
    _set_state(eng, D, C, seed=70, momentum=True)
    before = _state(eng)
    ref_eval = CLIP_SCALE * F.linear(F.batch_norm(feats, before[4].clone(), before[5].clone(), None, None, False, 0.1, 1e-5),
                                     before[0], before[1])
    pred = eng.probe_predict(feats, index=idx, scale=CLIP_SCALE)
    logits, loss = eng.probe_step(feats, idx, labels, lr=LR, momentum=MOM, weight_decay=WD, nesterov=True, scale=CLIP_SCALE)
    torch.cuda.synchronize()
    e = max_rel(pred, ref_eval[idx])
    print(f"predict B{B} D{D} C{C}: {e:.2e} (gate {GATE_OUT:g})")
    assert e <= GATE_OUT
    ref = _torch_step(before, feats, idx, labels, True, CLIP_SCALE, True, first=False)
    _check_step(f"step B{B} D{D} C{C}", eng, logits, loss, ref)


def test_an_ignored_label_leaves_the_mean_to_the_other_rows():
    B, D, C = 33, 64, 37
    eng = _engine(D, C)
    feats, idx, labels = _data(B, D, C, False, ignore=True)
    assert int((labels[idx] == -100).sum()) == 1
    _set_state(eng, D, C, momentum=True)
    before = _state(eng)
    logits, loss = eng.probe_step(feats, idx, labels, lr=LR, momentum=MOM, weight_decay=WD, scale=CLIP_SCALE)
    torch.cuda.synchronize()
    _check_step("ignore_index", eng, logits, loss, _torch_step(before, feats, idx, labels, True, CLIP_SCALE, False, first=False))


def test_state_carries_over_four_steps_without_compounding_tolerances():
    """Two epochs of two batches (8 and a ragged 5 of 13 rows): every step is compared with the torch step FROM THE ENGINE'S OWN
    STATE before it, so the gates are those of a single step.  Covers the first-step momentum rule (step 0 has no buffer to read),
    the running-statistics update and the ragged last batch."""
    D, C, N, bs = 64, 37, 13, 8
    eng = _engine(D, C)
    feats, _, labels = _data(N, D, C, False, seed=20, rows=N)
    _set_state(eng, D, C, seed=20)
    g = torch.Generator().manual_seed(5)
    step = 0
    for epoch in range(2):
        perm = torch.randperm(N, generator=g).cuda()
        for lo in range(0, N, bs):
            idx = perm[lo:lo + bs].contiguous()
            before = _state(eng)
            logits, loss = eng.probe_step(feats, idx, labels, lr=LR, momentum=MOM, weight_decay=WD, nesterov=True)
            torch.cuda.synchronize()
            ref = _torch_step(before, feats, idx, labels, True, 1.0, True, first=step == 0)
            _check_step(f"carry-over step {step} (batch {idx.numel()})", eng, logits, loss, ref)
            step += 1
    assert step == 4 and eng._steps == 4


def test_update_switch_off_leaves_the_state_and_adam_follows():
    from pevit_amd.engine import OptimPlan
    B, D, C = 33, 64, 37
    eng = _engine(D, C)
    feats, idx, labels = _data(B, D, C, False, seed=30)
    _set_state(eng, D, C, seed=30)
    before = _state(eng)
    p0, m0 = eng.params.clone(), eng.momentum.clone()
    logits, loss = eng.probe_step(feats, idx, labels, bn_training=True, scale=CLIP_SCALE, update=False)
    torch.cuda.synchronize()
    assert torch.equal(eng.params, p0) and torch.equal(eng.momentum, m0) and eng._steps == 0
    ref = _torch_step(before, feats, idx, labels, True, CLIP_SCALE, False, first=True, update=False)
    _check_step("update off", eng, logits, loss, ref, updated=False)
    # ... then Adam through the existing pevit_optim_step, under the gate of tests/test_gpu_optimizer.py on the engine's gradients
    gv = eng.grad_views()
    grads = [[gv["layers.0.weight"].detach().cpu().clone(), gv["layers.0.bias"].detach().cpu().clone()]]
    params0 = [before[0].cpu(), before[1].cpu()]
    hyp = [dict(lr=1e-3, weight_decay=1e-2)]
    plan = OptimPlan("adam", [dict(lr=1e-3, weight_decay=1e-2, beta1=0.9, beta2=0.999, eps=1e-8)],
                     torch.zeros(eng.n_params, dtype=torch.uint8), [0])
    eng.optimizer_step(plan)
    torch.cuda.synchronize()
    p32, s32 = og.run_reference("adam", params0, grads, [0, 0], torch.float32, hypers=hyp)
    p64, s64 = og.run_reference("adam", params0, grads, [0, 0], torch.float64, hypers=hyp)
    pv, mv, vv = eng.param_views(), eng.param_views(eng.momentum), eng.param_views(eng.exp_avg_sq)
    for i, n in enumerate(("layers.0.weight", "layers.0.bias")):
        og.gate(f"adam {n} p", pv[n].cpu(), p32[i], p64[i])
        og.gate(f"adam {n} exp_avg", mv[n].cpu(), s32["exp_avg"][i], s64["exp_avg"][i])
        og.gate(f"adam {n} exp_avg_sq", vv[n].cpu(), s32["exp_avg_sq"][i], s64["exp_avg_sq"][i])


@pytest.mark.parametrize("bce", [False, True], ids=["ce", "bce"])
def test_the_same_step_twice_gives_the_same_bits(bce):
    B, D, C = 128, 768, 211
    eng = _engine(D, C)
    feats, idx, labels = _data(B, D, C, bce, seed=40)
    outs = []
    for _ in range(2):
        _set_state(eng, D, C, seed=40, momentum=True)
        logits, loss = eng.probe_step(feats, idx, labels, lr=LR, momentum=MOM, weight_decay=WD, nesterov=True, scale=CLIP_SCALE)
        torch.cuda.synchronize()
        outs.append([logits.clone(), loss.clone(), eng.grads.clone(), eng.params.clone(), eng.momentum.clone(),
                     eng.running_mean.clone(), eng.running_var.clone()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_predict_matches_eval_mode_torch_and_rows_do_not_depend_on_their_neighbours():
    D, C, N = 512, 100, 300
    eng = _engine(D, C)
    feats = rnd(N + 20, D, seed=50, scale=1.5) + 0.3
    _set_state(eng, D, C, seed=50)
    W, b = eng.param_views()["layers.0.weight"], eng.param_views()["layers.0.bias"]
    ref_all = CLIP_SCALE * F.linear(F.batch_norm(feats, eng.running_mean.clone(), eng.running_var.clone(), None, None, False, 0.1, 1e-5), W, b)
    idx = torch.randperm(N + 20, generator=torch.Generator().manual_seed(51))[:N].cuda()
    by_index = eng.probe_predict(feats, index=idx, scale=CLIP_SCALE)
    by_range = eng.probe_predict(feats, first_row=7, count=N, scale=CLIP_SCALE)
    seven = eng.probe_predict(feats, index=idx[40:47].contiguous(), scale=CLIP_SCALE)
    torch.cuda.synchronize()
    e1, e2 = max_rel(by_index, ref_all[idx]), max_rel(by_range, ref_all[7:7 + N])
    print(f"probe_predict vs torch: index list {e1:.2e}, contiguous range {e2:.2e} (gate {GATE_OUT:g})")
    assert e1 <= GATE_OUT and e2 <= GATE_OUT
    assert torch.equal(seven, by_index[40:47])                          # a call of 7 and a call of 300: the same bits per row
    pos = {int(r): i for i, r in enumerate(idx.tolist())}
    shared = [r for r in range(7, 7 + N) if r in pos][:16]
    assert shared and all(torch.equal(by_range[r - 7], by_index[pos[r]]) for r in shared)


def test_cached_steps_equal_uncached_steps_on_the_tiny_tower():
    """3 steps of batch 8 on the tiny tower (method none): HipEngine.train_step on the images against encode_image on the same 8
    images as one chunk + pevit_probe_step.  Expected bit-identical: the features (encode_image runs the inference forms of the
    kernels the saving forward runs, which the predict path's tests hold to the same bits), hence everything the head reads; the
    two heads differ in summation order only (batch statistics, the logits' contraction over D, dW's over the batch).  Gates:
    logits and loss 1e-5, parameters after each step 1e-6; each step starts from the copied state."""
    from conftest import load_tiny_sd
    from pevit_amd.engine import HipEngine
    from pevit_amd.synth import ARCHS
    arch, C, B = ARCHS["tiny-128"], 10, 8
    sd = load_tiny_sd()
    engs = [HipEngine(arch, "none", C, B) for _ in range(2)]
    for e in engs:
        e.load_state_dict(sd)
    unc, cac = engs
    _set_state(cac, arch.embed_dim, C, seed=60)
    g = torch.Generator().manual_seed(61)
    for step in range(3):
        images = torch.randn((B, 3, arch.resolution, arch.resolution), generator=g).cuda()
        labels = torch.randint(0, C, (B,), generator=g).cuda()
        # both start from the cached engine's state
        unc.params.copy_(cac.params); unc.momentum.copy_(cac.momentum)
        unc.running_mean.copy_(cac.running_mean); unc.running_var.copy_(cac.running_var)
        unc._steps = cac._steps
        feats = cac.encode_image(images)
        assert torch.equal(feats, unc.visual_forward(images, save=True))
        l0, s0 = unc.train_step(images, labels, lr=LR, momentum=MOM, weight_decay=WD)
        l1, s1 = cac.probe_step(feats, torch.arange(B - 1, -1, -1).cuda(), labels, lr=LR, momentum=MOM, weight_decay=WD)
        torch.cuda.synchronize()
        figs = {"logits": (max_rel(l1.flip(0), l0), GATE_OUT), "loss": (max_rel(s1, s0), GATE_OUT),
                "params": (max_rel(cac.params, unc.params), GATE_STATE), "momentum": (max_rel(cac.momentum, unc.momentum), GATE_GRAD),
                "running_mean": (max_rel(cac.running_mean, unc.running_mean), GATE_STATE),
                "running_var": (max_rel(cac.running_var, unc.running_var), GATE_STATE)}
        print(f"cached vs uncached step {step}:", " ".join(f"{k} {v:.2e}" for k, (v, _) in figs.items()))
        for k, (v, gate) in figs.items():
            assert v <= gate, f"step {step}: {k} max_rel {v:.3e} over the gate {gate:g}"


def test_a_bound_context_refuses_a_batch_over_max_batch_and_null_pointers():
    import ctypes as C
    from pevit_amd import _lib
    eng = _engine(64, 37)
    _set_state(eng, 64, 37)
    a = _lib.PevitProbeArgs()
    a.batch, a.scale = eng.max_batch + 1, 1.0
    assert eng.lib.pevit_probe_step(eng._ctx, None, C.byref(a)) != 0
    assert f"exceeds max_batch {eng.max_batch}".encode() in eng.lib.pevit_last_error()
    a.batch = 8
    assert eng.lib.pevit_probe_step(eng._ctx, None, C.byref(a)) != 0 and b"null argument" in eng.lib.pevit_last_error()
    feats, idx, labels = _data(8, 64, 37, False)
    with pytest.raises(_lib.PevitError, match="outside"):
        eng.probe_step(feats, idx[:1].contiguous(), labels)
    with pytest.raises(_lib.PevitError, match="outside the 13 feature rows"):
        eng.probe_predict(feats, first_row=10, count=4)


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    from conftest import load_tiny_sd
    p = tmp_path_factory.mktemp("ckpt") / "tiny.pt"
    torch.save(load_tiny_sd(), p)
    return p


def _end_to_end(ckpt, cache, monkeypatch):
    """full_model_finetune on a synthetic set for 2 epochs without tuning: (best score, the epoch's index batches, the raw outputs
    every train epoch and every validation handed to the metric)."""
    from test_mirror_api import tiny_config
    from pevit_amd.evaluation import _harness as h, full_model_finetune as fm
    from pevit_amd.evaluation.dataloader import TensorLoader, construct_dataloader
    cfg = tiny_config(ckpt, classes=5)
    cfg.DATASET.DATASET, cfg.DATASET.SYNTHETIC_SIZES, cfg.DATASET.LOADER_BATCH_SIZE = "synthetic", (40, 10), 16
    cfg.TRAIN.IMAGE_SIZE = [48, 48]
    cfg.TRAIN.FREEZE_IMAGE_BACKBONE, cfg.TRAIN.CACHE_FEATURES = True, cache
    cfg.TRAIN.END_EPOCH, cfg.TRAIN.EXTRA_FINAL_TRAIN_EPOCH = 2, 0
    cfg.GPUS = (0,)
    fm.clear_feature_cache()
    h._BACKBONES.clear()                 # both runs build their model afresh: a re-used backbone draws less from the generator
    batches, scored = [], []
    real_iter, real_score = TensorLoader.iter_indices, h._score

    def iter_indices(self):
        for sel in real_iter(self):
            if self.shuffle:
                batches.append(sel.tolist())
            yield sel

    def score(metric, outputs, targets):
        scored.append(torch.cat(outputs).detach().float().cpu())
        return real_score(metric, outputs, targets)
    with monkeypatch.context() as m:
        m.setattr(TensorLoader, "iter_indices", iter_indices)
        m.setattr(h, "_score", score)
        torch.manual_seed(0)
        tr, va, te = construct_dataloader(cfg)
        best, info = fm.full_model_finetune(tr, va, te, True, 0.01, 1e-4, cfg)
    encoded = sum(c.encoded for sets in fm._FEATURES.values() for c in sets.values())
    fm.clear_feature_cache()
    return best, batches, scored, info, encoded


def test_end_to_end_cached_equals_uncached(ckpt, monkeypatch):
    """Same seed, same index batches, per-epoch outputs within 1e-4 of the largest magnitude (the head gate of 1e-5 with room for
    the steps of 2 epochs), the same best score."""
    b0, batches0, scored0, info0, enc0 = _end_to_end(ckpt, False, monkeypatch)
    b1, batches1, scored1, info1, enc1 = _end_to_end(ckpt, True, monkeypatch)
    assert enc0 == 0 and enc1 == 40 + 10                         # every image of the run once: 40 train + val rows, 10 test rows
    assert batches0 == batches1 and len(batches0) == 2 * 3       # 2 epochs x 40 rows in batches of 16
    assert len(scored0) == len(scored1) == 4                     # per epoch: the train outputs, the validation outputs
    for i, (a, b) in enumerate(zip(scored0, scored1)):
        assert a.shape == b.shape
        err = float((a - b).abs().max() / a.abs().max())
        print(f"end to end, {'train' if i % 2 == 0 else 'validation'} outputs of epoch {i // 2}: cached vs uncached {err:.2e} (gate 1e-4)")
        assert err <= 1e-4
    assert b0 == b1 and info0["n_trainable_params"] == info1["n_trainable_params"] == 5 * 64 + 5
    assert np.allclose(info0["best_logits"], info1["best_logits"], atol=1e-4)


def _two_sweep_runs(ckpt, cache, monkeypatch):
    """Two sweep runs (two weight decays) of the probe AT A TIME, as hyperparameter_sweep starts them by default: (scores, the raw
    outputs every run handed to the metric, per run; rows encoded; rows of the train and val views)."""
    import threading
    from test_mirror_api import tiny_config
    from pevit_amd.evaluation import _harness as h, full_model_finetune as fm
    from pevit_amd.evaluation.dataloader import construct_dataloader
    cfg = tiny_config(ckpt, classes=5)
    cfg.DATASET.DATASET, cfg.DATASET.SYNTHETIC_SIZES, cfg.DATASET.LOADER_BATCH_SIZE = "synthetic", (40, 10), 16
    cfg.TRAIN.IMAGE_SIZE = [48, 48]
    cfg.TRAIN.FREEZE_IMAGE_BACKBONE, cfg.TRAIN.CACHE_FEATURES = True, cache
    cfg.TRAIN.END_EPOCH, cfg.TRAIN.LR = 2, 0.01
    cfg.GPUS = (0,)
    fm.clear_feature_cache()
    h._BACKBONES.clear()
    scored, real_score, lock = {}, h._score, threading.Lock()

    def score(metric, outputs, targets):
        with lock:
            scored.setdefault(threading.current_thread().name, []).append(torch.cat(outputs).detach().float().cpu())
        return real_score(metric, outputs, targets)
    with monkeypatch.context() as m:
        m.setattr(h, "_score", score)
        torch.manual_seed(0)
        tr, va, _ = construct_dataloader(cfg)
        scores = h.run_tasks(fm.train_task, tr, va, cfg, [1e-4, 1e-2], 2)
    encoded = sum(c.encoded for sets in fm._FEATURES.values() for c in sets.values())
    fm.clear_feature_cache()
    return scores, scored, encoded, len(tr.dataset) + len(va.dataset)


def test_two_concurrent_sweep_runs_share_one_fill_of_the_cache(ckpt, monkeypatch):
    """The default sweep runs two train_task calls at a time, each in a thread with its own stream and engine, on ONE cache: every
    row of the train and val views is encoded once (not once per run), and each run computes what the same concurrent run computes
    uncached -- the same scores, per-epoch outputs within the end-to-end gate of 1e-4 of the largest magnitude."""
    s0, scored0, enc0, n0 = _two_sweep_runs(ckpt, False, monkeypatch)
    s1, scored1, enc1, n1 = _two_sweep_runs(ckpt, True, monkeypatch)
    assert None not in s0 and None not in s1                     # (run_tasks turns a run's exception into a None score)
    assert enc0 == 0 and enc1 == n1 == n0
    assert sorted(scored0) == sorted(scored1) == ["sweep-run-0", "sweep-run-1"]
    for run in sorted(scored0):
        assert len(scored0[run]) == len(scored1[run]) == 4       # per epoch: the train outputs, the validation outputs
        for i, (a, b) in enumerate(zip(scored0[run], scored1[run])):
            assert a.shape == b.shape
            err = float((a - b).abs().max() / a.abs().max())
            print(f"{run}, {'train' if i % 2 == 0 else 'validation'} outputs of epoch {i // 2}: cached vs uncached {err:.2e} (gate 1e-4)")
            assert err <= 1e-4
    assert s0 == s1
