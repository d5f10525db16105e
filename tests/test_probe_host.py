"""CPU-side checks of the linear probe: the two new C entries are exported, declared and typed; contexts and shapes outside the
kernels' limits are refused on the host before any launch; ``full_model_finetune.Classifier`` freezes what the reference freezes and
computes the reference's forward; the pure route selection; the cached route's index batches are the loader's own; the feature
cache encodes every row once; the command layers its config and writes the reference's file."""
import ctypes as C
import importlib
import json
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from conftest import ROOT, load_tiny_sd, max_rel

from test_mirror_api import tiny_config

from pevit_amd import _lib
from pevit_amd.config import default_config
from pevit_amd.evaluation.dataloader import TensorLoader, _Tensors, _View

P = C.c_void_p
ENTRIES = {
    "pevit_probe_step": (["pevit_ctx*", "void*", "const pevit_probe_args*"], [P, P, C.POINTER(_lib.PevitProbeArgs)]),
    "pevit_probe_predict": (["pevit_ctx*", "void*", "const pevit_probe_predict_args*"], [P, P, C.POINTER(_lib.PevitProbePredictArgs)]),
}
STRUCTS = {"pevit_probe_args": _lib.PevitProbeArgs, "pevit_probe_predict_args": _lib.PevitProbePredictArgs}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    p = tmp_path_factory.mktemp("ckpt") / "tiny.pt"
    torch.save(load_tiny_sd(), p)
    return p


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_probe_entries_are_exported_declared_and_typed(lib, name):
    ctypes_args = ENTRIES[name][1]
    assert hasattr(lib, name), f"{name} is not exported by the library"
    header = open(os.path.join(ROOT, "include", "pevit_hip.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/pevit_hip.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert [a.rsplit(" ", 1)[0] for a in args] == ENTRIES[name][0]
    res, argtypes = _lib.SIGNATURES[name]
    assert res is C.c_int and argtypes == ctypes_args
    fn = getattr(lib, name)
    assert fn.restype is C.c_int and list(fn.argtypes) == argtypes


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_the_ctypes_structs_have_the_header_fields_in_order(name):
    header = open(os.path.join(ROOT, "include", "pevit_hip.h")).read()
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [part.strip().split()[-1].lstrip("*") for part in decl.split(",")]
    assert fields == [f[0] for f in STRUCTS[name]._fields_]


def _step_args(batch=8):
    a = _lib.PevitProbeArgs()
    a.batch, a.scale = batch, 1.0
    return a


def _predict_args(count=8):
    a = _lib.PevitProbePredictArgs()
    a.count, a.scale = count, 1.0
    return a


def _ctx(lib, out_dim=64, method=4, classes=10):
    d = _lib.PevitDims(128, 2, 16, 48, out_dim, method, 4, classes)
    ctx = C.c_void_p()
    assert lib.pevit_ctx_create(C.byref(d), C.byref(ctx)) == 0, lib.pevit_last_error()
    return ctx


def _both(lib, ctx, batch=8):
    yield "probe_step", lib.pevit_probe_step(ctx, None, C.byref(_step_args(batch)))
    yield "probe_predict", lib.pevit_probe_predict(ctx, None, C.byref(_predict_args(batch)))


def test_an_unbound_context_is_refused(lib):
    ctx = _ctx(lib)
    for who, rc in _both(lib, ctx):
        assert rc != 0 and b"not bound" in lib.pevit_last_error(), who
    lib.pevit_ctx_destroy(ctx)


def test_a_text_context_is_refused(lib):
    d = _lib.PevitTextDims(128, 2, 16, 1000, 64, 0)
    ctx = C.c_void_p()
    assert lib.pevit_text_create(C.byref(d), C.byref(ctx)) == 0, lib.pevit_last_error()
    for who, rc in _both(lib, ctx):
        assert rc != 0 and b"text context" in lib.pevit_last_error(), who
    lib.pevit_ctx_destroy(ctx)


@pytest.mark.parametrize("method", [0, 1, 2, 3])
def test_a_context_with_adapters_is_refused(lib, method):
    ctx = _ctx(lib, method=method)
    for who, rc in _both(lib, ctx):
        assert rc != 0 and b"PEVIT_NONE" in lib.pevit_last_error(), who
    lib.pevit_ctx_destroy(ctx)


@pytest.mark.parametrize("out_dim,classes,batch,word", [(72, 10, 8, b"multiple of 16 in [16, 1024]"), (1040, 10, 8, b"multiple of 16 in [16, 1024]"),
                                                        (64, 1025, 8, b"classes outside [1, 1024]")])
def test_shapes_outside_the_limits_are_refused_before_any_launch(lib, out_dim, classes, batch, word):
    """The context is unbound, so a refusal that names the limit was decided before anything could have been launched."""
    ctx = _ctx(lib, out_dim=out_dim, classes=classes)
    for who, rc in _both(lib, ctx, batch):
        assert rc != 0 and word in lib.pevit_last_error(), (who, lib.pevit_last_error())
    lib.pevit_ctx_destroy(ctx)


def test_a_batch_below_two_is_refused_by_the_step_and_no_rows_by_predict(lib):
    ctx = _ctx(lib)
    assert lib.pevit_probe_step(ctx, None, C.byref(_step_args(1))) != 0
    assert b"batch 1 must be at least 2" in lib.pevit_last_error()
    assert lib.pevit_probe_predict(ctx, None, C.byref(_predict_args(0))) != 0
    assert b"at least 1" in lib.pevit_last_error()
    assert lib.pevit_probe_step(ctx, None, None) != 0 and b"null argument struct" in lib.pevit_last_error()
    lib.pevit_ctx_destroy(ctx)


# ---- the Classifier on a tiny CPU model ------------------------------------------------------------------------------------------
def _classifier(ckpt, **train):
    from pevit_amd.evaluation import full_model_finetune as fm
    cfg = tiny_config(ckpt)
    cfg.TRAIN.FREEZE_IMAGE_BACKBONE = True
    cfg.TRAIN.LR, cfg.TRAIN.WD = 0.1, 1e-3
    for k, v in train.items():
        setattr(cfg.TRAIN, k, v)
    return cfg, fm.Classifier(cfg, 0)


def test_only_the_head_trains_under_a_frozen_backbone(ckpt):
    _, clf = _classifier(ckpt)
    assert [n for n, p in clf.named_parameters() if p.requires_grad] == ["layers.0.weight", "layers.0.bias"]
    assert clf.backbone.visual.method == "none"
    assert not any(p.requires_grad for n, p in clf.named_parameters() if n.startswith("backbone.visual"))


def test_full_fine_tuning_is_refused_with_what_is_not_built(ckpt):
    from pevit_amd.evaluation import full_model_finetune as fm
    cfg = tiny_config(ckpt)
    cfg.TRAIN.FREEZE_IMAGE_BACKBONE = False
    with pytest.raises(NotImplementedError, match="full fine-tuning.*not built"):
        fm.Classifier(cfg, 0)


@pytest.mark.parametrize("init,want", [("none", 1.0), ("clip", 1 / 0.07), ("ln_cls", math.log(10))])
def test_the_forward_scales_the_head_like_the_reference(ckpt, init, want):
    _, clf = _classifier(ckpt, LOGIT_SCALE_INIT=init)
    assert abs(clf.scale() - want) <= 1e-6 * want
    g = torch.Generator().manual_seed(1)
    feat = torch.randn((6, 64), generator=g) * 1.5 + 0.3
    with torch.no_grad():
        clf.layers[0].weight.copy_(torch.randn((10, 64), generator=g) * 0.2); clf.layers[0].bias.copy_(torch.randn(10, generator=g))
    clf.train()
    bn = nn.BatchNorm1d(64, affine=False)
    ref = clf.logit_scale.exp() * F.linear(bn(feat), clf.layers[0].weight, clf.layers[0].bias)
    out = clf.head(feat)
    assert max_rel(out.detach(), ref.detach()) <= 1e-6
    assert torch.equal(clf.channel_bn.running_mean, bn.running_mean)
    # the image-to-logits engine calls carry no scale: they are the module's forward only at scale 1
    assert clf._fusable_step(nn.CrossEntropyLoss()) == (init == "none")


# ---- route selection ---------------------------------------------------------------------------------------------------------------
def _head_and_layout():
    lin = nn.Linear(8, 3)
    return lin, [(lin.weight, 0, lin.weight.numel()), (lin.bias, lin.weight.numel(), lin.bias.numel())]


def test_route_selection_follows_the_table():
    from pevit_amd.evaluation.full_model_finetune import select_probe_route as route
    lin, layout = _head_and_layout()
    ps = list(lin.parameters())
    ce, bce = nn.CrossEntropyLoss(), nn.BCEWithLogitsLoss()
    sgd = torch.optim.SGD(ps, lr=0.1, momentum=0.9, weight_decay=1e-3, nesterov=True)
    assert route(ce, sgd, layout=layout) == "fused" and route(bce, sgd, layout=layout) == "fused"
    two = torch.optim.SGD([dict(params=[lin.weight], weight_decay=1e-3), dict(params=[lin.bias], weight_decay=0.0)], lr=0.1, momentum=0.9)
    assert route(ce, two, layout=layout) == "plan"
    assert route(ce, torch.optim.Adam(ps, lr=1e-3), layout=layout) == "plan"
    assert route(ce, torch.optim.AdamW(ps, lr=1e-3), layout=layout) == "plan"
    assert route(ce, torch.optim.Adam(ps, lr=1e-3), layout=None) == "autograd"                  # TRAIN.FUSED_OPTIMIZER False
    assert route(ce, torch.optim.RMSprop(ps, lr=1e-3), layout=layout) == "autograd"
    assert route(ce, sgd, layout=layout, trainable_logit_scale=True) == "autograd"
    assert route(ce, sgd, layout=layout, normalize=True) == "autograd"
    assert route(ce, sgd, layout=layout, has_channel_bn=False, bn_momentum=None, bn_eps=None) == "autograd"
    assert route(ce, sgd, layout=layout, bn_momentum=0.2) == "autograd"
    assert route(ce, sgd, layout=layout, bn_eps=1e-3) == "autograd"
    assert route(nn.CrossEntropyLoss(label_smoothing=0.1), sgd, layout=layout) == "autograd"
    assert route(nn.CrossEntropyLoss(weight=torch.ones(3)), sgd, layout=layout) == "autograd"
    assert route(nn.BCEWithLogitsLoss(pos_weight=torch.ones(3)), sgd, layout=layout) == "autograd"
    assert route(ce, sgd, layout=layout, soft_labels=True) == "autograd"
    assert route(nn.MSELoss(), sgd, layout=layout) == "autograd"
    assert route(ce, torch.optim.SGD(ps, lr=0.1, momentum=0.9, dampening=0.1), layout=layout) == "autograd"


def test_the_classifier_hands_its_own_state_to_the_route_selection(ckpt):
    from pevit_amd.optim import build_optimizer

    class _Cache:
        labels = torch.zeros(4, dtype=torch.int64)
    for train, want in (({}, "fused"), (dict(OPTIMIZER="adam"), "plan"), (dict(TRAINABLE_LOGIT_SCALE=True), "autograd"),
                        (dict(NORMALIZE_VISUAL_FEATURE=True), "autograd"), (dict(USE_CHANNEL_BN=False), "autograd"),
                        (dict(OPTIMIZER="adam", FUSED_OPTIMIZER=False), "autograd")):
        cfg, clf = _classifier(ckpt, **train)
        route, plan = clf.probe_route(nn.CrossEntropyLoss(), build_optimizer(cfg, clf), _Cache)
        assert route == want, (train, route)
        assert (plan is not None) == (want == "plan")


# ---- index batches and the cache ----------------------------------------------------------------------------------------------------
def _numbered_set(n=23):
    """images whose first pixel, and labels, are their own row numbers"""
    images = torch.zeros((n, 3, 2, 2)); images[:, 0, 0, 0] = torch.arange(n).float()
    return _Tensors(images, torch.arange(n))


@pytest.mark.parametrize("seed", [0, 7])
def test_cached_index_batches_are_the_loaders_own(seed):
    from pevit_amd.evaluation.full_model_finetune import epoch_index_batches
    full = _numbered_set()
    loader = TensorLoader(_View(full, [1, 2, 3, 5, 8, 13, 21, 0, 4, 6, 7]), batch_size=4, shuffle=True)
    torch.manual_seed(seed)
    want = [y.tolist() for _ in range(2) for _, y in loader]               # labels are row numbers
    state_want = torch.get_rng_state()
    torch.manual_seed(seed)
    got = [sel.tolist() for _ in range(2) for sel in epoch_index_batches(loader)]
    assert got == want and [len(b) for b in got] == [4, 4, 3, 4, 4, 3]
    assert torch.equal(torch.get_rng_state(), state_want)
    assert got[:3] != got[3:]                                                # a new shuffle every epoch


def test_every_row_is_encoded_once_and_only_rows_in_the_views():
    from pevit_amd.evaluation import full_model_finetune as fm
    from pevit_amd.evaluation._harness import merge_trainval_loader
    fm.clear_feature_cache()
    full = _numbered_set(40)
    keep = list(range(0, 30))                                # 10 rows of the archive are in no view
    tr = TensorLoader(_View(full, keep[:24]), batch_size=8, shuffle=True)
    va = TensorLoader(_View(full, keep[24:]), batch_size=8, shuffle=False)
    calls, seen = [], []

    def encode(sel):
        calls.append(int(sel.numel())); seen.extend(sel.tolist())
        return full.images[sel, 0, 0, 0].view(-1, 1).repeat(1, 16) * 2.0           # feature = 2 x row number

    key = ("ckpt", "bf16", None)
    for run in range(2):
        for loader in (tr, va):
            full_, rows = fm.loader_rows(loader)
            assert full_ is full
            cache = fm.feature_cache(key, full_, 16, "cpu").ensure(rows, encode)
    assert sorted(seen) == keep and cache.encoded == 30 and int(cache.have.sum()) == 30
    merged = TensorLoader(full, batch_size=8, shuffle=True)                 # what merge_trainval_loader builds when the views cover the set
    assert fm.feature_cache(key, full, 16, "cpu") is cache
    cache.ensure(fm.loader_rows(merged)[1], encode)
    assert sorted(seen) == list(range(40)) and cache.encoded == 40          # ten new rows, none twice
    assert torch.equal(cache.feats[:, 0], torch.arange(40).float() * 2.0) and torch.equal(cache.labels, full.labels)
    assert all(c <= fm.ENCODE_CHUNK for c in calls)
    # the merged loader of the harness is over the same set object
    full2 = _numbered_set(30)
    t2, v2 = TensorLoader(_View(full2, keep[:24]), batch_size=8), TensorLoader(_View(full2, keep[24:]), batch_size=8)
    assert fm.loader_rows(merge_trainval_loader(t2, v2))[0] is full2
    # another checkpoint, weight format or normalisation drops what was cached
    other = fm.feature_cache(("ckpt2", "bf16", None), full, 16, "cpu")
    assert other is not cache and other.encoded == 0 and key not in fm._FEATURES
    assert fm.loader_rows(torch.utils.data.DataLoader(torch.utils.data.TensorDataset(torch.zeros(4, 1)))) is None
    fm.clear_feature_cache()


def test_two_concurrent_runs_encode_every_row_once():
    """Two sweep runs reach an empty cache at the same moment (the default TRAIN.SWEEP_CONCURRENCY is 2): the second waits for
    the first one's fill and finds the rows present -- one cache object, every row encoded once, and no row marked present
    before its features are written.  The second thread asks for the cache while the first is INSIDE its encoder."""
    import threading
    from pevit_amd.evaluation import full_model_finetune as fm
    fm.clear_feature_cache()
    full = _numbered_set(40)
    rows = torch.arange(30)
    key = ("ckpt", "bf16", None)
    inside, second_started = threading.Event(), threading.Event()
    count_lock, seen, caches, early, errors = threading.Lock(), [], {}, [], []

    def encode(sel):
        inside.set()
        assert second_started.wait(30)
        with count_lock:
            seen.extend(sel.tolist())
        return full.images[sel, 0, 0, 0].view(-1, 1).repeat(1, 16) * 2.0 + 1.0     # never the zero a row holds before its fill

    def run(name):
        try:
            if name == "second":
                assert inside.wait(30)
                second_started.set()
            cache = caches[name] = fm.feature_cache(key, full, 16, "cpu")
            cache.ensure(rows, encode)
            present = cache.have.nonzero().flatten()
            early.append(bool((cache.feats[present] == 0).any()))             # what this run would read right after cached()
        except BaseException as e:                                            # (a thread's assertion must reach the test)
            errors.append(e)
            second_started.set()
    threads = [threading.Thread(target=run, args=(n,)) for n in ("first", "second")]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not errors and not any(t.is_alive() for t in threads)
    assert caches["first"] is caches["second"]
    assert sorted(seen) == rows.tolist() and caches["first"].encoded == 30
    assert early == [False, False]
    assert torch.equal(caches["first"].feats[:30, 0], torch.arange(30).float() * 2.0 + 1.0)
    fm.clear_feature_cache()


# ---- the command -------------------------------------------------------------------------------------------------------------------
NINE_KEYS = {"model_name", "dataset_name", "num_trainable_params", "num_params", "num_visual_params", "num_backbone_params",
             "n_shot", "rnd_seeds", "predictions"}


def _yamls(tmp_path):
    ds = tmp_path / "ds.yaml"
    ds.write_text("DATASET:\n  DATASET: 'synthetic'\n  NUM_CLASSES: 7\nTEST:\n  METRIC: 'accuracy'\n")
    model = tmp_path / "model.yaml"
    model.write_text("MODEL:\n  NAME: 'ViT-B/32'\n  SPEC:\n    EMBED_DIM: 512\nTRAIN:\n  FREEZE_IMAGE_BACKBONE: true\n  END_EPOCH: 10\n"
                     "  EXTRA_FINAL_TRAIN_EPOCH: 40\n")
    return ds, model


def test_command_layers_the_config_and_writes_the_reference_file(tmp_path, monkeypatch):
    from pevit_amd.commands import linear_probe as cmd
    ds, model = _yamls(tmp_path)
    seen = {}

    def fake_entry(tr, va, te, no_tuning, lr, l2, cfg):
        seen.update(no_tuning=no_tuning, lr=lr, l2=l2, shots=cfg.DATASET.NUM_SAMPLES_PER_CLASS, merge=cfg.DATASET.MERGE_TRAIN_VAL_FINAL_RUN,
                    freeze=cfg.TRAIN.FREEZE_IMAGE_BACKBONE, n=(len(tr.dataset), len(va.dataset), len(te.dataset)))
        return 12.5, {"best_logits": np.full((2, 7), 0.123456789), "n_trainable_params": 10, "n_params": 20, "n_visual_params": 7,
                      "n_backbone_params": 5}

    monkeypatch.setattr(cmd, "config", default_config())
    acc, _ = cmd.main(["--ds", str(ds), "--model", str(model), "--no-tuning", "True", "--lr", "0.1", "--l2", "1e-6",
                       "DATASET.NUM_SAMPLES_PER_CLASS", "1", "OUTPUT_DIR", str(tmp_path / "out"), "TRAIN.IMAGE_SIZE", "[8, 8]",
                       "DATASET.SYNTHETIC_SIZES", "(70, 14)"], entry=fake_entry)
    assert acc == 12.5 and seen["no_tuning"] is True and seen["lr"] == 0.1 and seen["l2"] == 1e-6 and seen["freeze"] is True
    assert seen["shots"] == 2 and seen["merge"] is False                    # the 1 -> 2 shot rule
    assert seen["n"][0] + seen["n"][1] == 14 and seen["n"][2] == 14         # 2 shots x 7 classes
    path = tmp_path / "out" / "predictions" / "linear_probe_1" / "seed0_synthetic.json"      # named before the rule, as the reference
    j = json.loads(path.read_text())
    assert set(j) == NINE_KEYS and j["n_shot"] == 2 and j["rnd_seeds"] == [0] and j["model_name"] == "ViT-B/32"
    assert j["dataset_name"] == "synthetic" and j["num_trainable_params"] == 10 and j["num_visual_params"] == 7
    assert j["predictions"][0][0][0] == 0.123457 and np.asarray(j["predictions"]).shape == (1, 2, 7)


def test_emulate_zeroshot_sets_the_four_fields_and_submit_is_refused(tmp_path, monkeypatch):
    from pevit_amd.commands import linear_probe as cmd
    ds, model = _yamls(tmp_path)
    cfg = default_config()
    monkeypatch.setattr(cmd, "config", cfg)
    args, exp = cmd.prepare(["--ds", str(ds), "--model", str(model), "--emulate-zeroshot", "True", "DATASET.NUM_SAMPLES_PER_CLASS", "5"])
    assert args.no_tuning is True and exp == "linear_probe_0"
    assert (cfg.TRAIN.END_EPOCH, cfg.TRAIN.EXTRA_FINAL_TRAIN_EPOCH, cfg.DATASET.NUM_SAMPLES_PER_CLASS, cfg.TRAIN.EMULATE_ZERO_SHOT) == \
        (1, 0, 0, True)
    monkeypatch.setattr(cmd, "config", default_config())
    args, exp = cmd.prepare(["--ds", str(ds), "--model", str(model)])
    assert args.no_tuning is False and exp == "linear_probe_full" and not args.emulate_zeroshot
    monkeypatch.setattr(cmd, "config", default_config())
    with pytest.raises(SystemExit):
        cmd.prepare(["--ds", str(ds), "--model", str(model), "--submit-predictions"])


def test_the_reference_import_paths_resolve():
    alias = importlib.import_module("vision_benchmark.commands.linear_probe")
    from pevit_amd.commands import linear_probe as cmd
    assert alias.main is cmd.main
    mod = importlib.import_module("vision_benchmark.evaluation.full_model_finetune")
    for name in ("Classifier", "train_task", "train_one", "validate", "hyperparameter_sweep", "hyperparameter_sweep_lr",
                 "merge_trainval_loader", "full_model_finetune"):
        assert hasattr(mod, name), name
    assert os.path.isfile(os.path.join(ROOT, "vision_benchmark", "commands", "linear_probe.py"))
    assert default_config().TRAIN.CACHE_FEATURES is True
