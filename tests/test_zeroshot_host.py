"""CPU-side checks of the zero-shot path's boundary: the five new C entries are exported, declared and typed; unbound and text
contexts are refused; the head's limits are refused on the host before any launch; ``clip_zeroshot_evaluator`` computes the
reference's formula; the command scores a feature file in the reference's format without building a model and writes the
reference's result file."""
import ctypes as C
import importlib
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, max_rel

from pevit_amd import _lib
from pevit_amd.config import default_config

P, I, F = C.c_void_p, C.c_int, C.c_float

# name -> (C argument types after whitespace normalisation, ctypes argument types)
ENTRIES = {
    "pevit_encode_image": (["pevit_ctx*", "void*", "const float*", "float*", "int"], [P, P, P, P, I]),
    "pevit_encode_image_u8": (["pevit_ctx*", "void*", "const uint8_t*", "float*", "int"], [P, P, P, P, I]),
    "pevit_zeroshot": (["pevit_ctx*", "void*", "const float*", "const float*", "int", "float", "float*", "float*", "float*", "int"],
                       [P, P, P, P, I, F, P, P, P, I]),
    "pevit_zeroshot_u8": (["pevit_ctx*", "void*", "const uint8_t*", "const float*", "int", "float", "float*", "float*", "float*",
                           "int"], [P, P, P, P, I, F, P, P, P, I]),
    "pevit_op_zeroshot_head": (["void*", "const float*", "const float*", "float", "float*", "float*", "int", "int", "int"],
                               [P, P, P, F, P, P, I, I, I]),
}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_zeroshot_entries_are_exported_declared_and_typed(lib, name):
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


def test_an_unbound_context_refuses_the_image_entries(lib):
    d = _lib.PevitDims(128, 2, 16, 48, 64, 4, 4, 10)               # method none
    ctx = C.c_void_p()
    assert lib.pevit_ctx_create(C.byref(d), C.byref(ctx)) == 0
    assert lib.pevit_encode_image(ctx, None, None, None, 1) != 0
    assert b"not bound" in lib.pevit_last_error()
    assert lib.pevit_zeroshot(ctx, None, None, None, 5, 100.0, None, None, None, 1) != 0
    assert b"not bound" in lib.pevit_last_error()
    assert lib.pevit_encode_image_u8(ctx, None, None, None, 1) != 0
    assert b"pevit_set_input_norm" in lib.pevit_last_error()
    assert lib.pevit_zeroshot_u8(ctx, None, None, None, 5, 100.0, None, None, None, 1) != 0
    assert b"pevit_set_input_norm" in lib.pevit_last_error()
    lib.pevit_ctx_destroy(ctx)


def test_a_text_context_refuses_the_image_entries(lib):
    d = _lib.PevitTextDims(128, 2, 16, 1000, 64, 0)
    ctx = C.c_void_p()
    assert lib.pevit_text_create(C.byref(d), C.byref(ctx)) == 0, lib.pevit_last_error()
    for call in (lambda: lib.pevit_encode_image(ctx, None, None, None, 1),
                 lambda: lib.pevit_encode_image_u8(ctx, None, None, None, 1),
                 lambda: lib.pevit_zeroshot(ctx, None, None, None, 5, 100.0, None, None, None, 1),
                 lambda: lib.pevit_zeroshot_u8(ctx, None, None, None, 5, 100.0, None, None, None, 1)):
        assert call() != 0
        assert b"text context" in lib.pevit_last_error()
    lib.pevit_ctx_destroy(ctx)


@pytest.mark.parametrize("D,Cc,both_null,word", [(64, 0, False, b"classes"), (64, 1025, False, b"classes"), (12, 5, False, b"multiple of 8"),
                                                  (64, 5, True, b"both outputs")])
def test_the_head_refuses_what_is_outside_its_limits_before_any_launch(lib, D, Cc, both_null, word):
    """Host memory stands in for the operands: a refusal reads no pointer and launches nothing (there is no GPU here)."""
    feat = (C.c_float * 2048)(); text = (C.c_float * 2048)(); out = (C.c_float * 2048)()
    a = lambda b: C.c_void_p(C.addressof(b) + (-C.addressof(b)) % 16)          # 16-byte aligned inside the buffer
    rc = lib.pevit_op_zeroshot_head(None, a(feat), a(text), 100.0, None if both_null else a(out), None, 1, D, Cc)
    assert rc != 0
    assert word in lib.pevit_last_error(), lib.pevit_last_error()


# ---- the host evaluator ----------------------------------------------------------------------------------------------------------
def _seeded(N=23, D=64, Cc=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn((N, D), generator=g) * 3
    text = torch.nn.functional.normalize(torch.randn((Cc, D), generator=g).double(), dim=1).float()        # unit rows
    return feat, text


def _f64_probs(feat, text_dc):
    f = feat.double()
    f = f / f.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return (100.0 * f @ text_dc.double()).softmax(dim=-1)


def test_evaluator_computes_the_reference_formula_and_counts_accuracy():
    from pevit_amd.evaluation import clip_zeroshot_evaluator
    feat, text = _seeded()
    text_dc = text.t().contiguous()                                  # (D, C), the reference's layout
    want = _f64_probs(feat, text_dc)
    labels = want.argmax(1).clone()
    labels[::4] = (labels[::4] + 1) % text.shape[0]                  # 6 of 23 wrong by construction
    cfg = default_config()
    cfg.TEST.METRIC = "accuracy"
    result, probs, name = clip_zeroshot_evaluator(feat.numpy(), text_dc.numpy(), labels.numpy(), cfg)
    assert name == "accuracy" and tuple(probs.shape) == (23, 7)
    err = max_rel(probs, want)
    print(f"clip_zeroshot_evaluator vs f64: max_rel {err:.3e} (gate 1e-5)")
    assert err <= 1e-5
    hand = sum(int(want[i].argmax()) == int(labels[i]) for i in range(23)) / 23
    assert hand == 17 / 23 and abs(result - hand) < 1e-12
    # (N, 1) labels, as the reference's extract_feature stacks them, are squeezed
    result2, _, _ = clip_zeroshot_evaluator(feat.numpy(), text_dc.numpy(), labels.numpy()[:, None], cfg)
    assert result2 == result


def test_evaluator_scores_multi_hot_labels_with_the_11_point_map():
    from pevit_amd.evaluation import clip_zeroshot_evaluator
    from pevit_amd.evaluation.metric import map_11_points
    feat, text = _seeded(N=30, Cc=5, seed=3)
    text_dc = text.t().contiguous()
    g = torch.Generator().manual_seed(4)
    multi = (torch.rand((30, 5), generator=g) < 0.4).long()
    multi[:, 0] = 1 - multi[:, 1]                                    # every class has positives
    cfg = default_config()
    cfg.TEST.METRIC = "11point_mAP"
    result, probs, name = clip_zeroshot_evaluator(feat.numpy(), text_dc.numpy(), multi.numpy(), cfg)
    assert name == "map_11_points" and 0.0 < result <= 1.0
    assert result == map_11_points(multi.numpy(), probs.numpy())


# ---- the command on a feature file -----------------------------------------------------------------------------------------------
NINE_KEYS = {"model_name", "dataset_name", "num_trainable_params", "num_params", "num_visual_params", "num_backbone_params",
             "n_shot", "rnd_seeds", "predictions"}


def test_command_scores_a_feature_file_and_writes_the_reference_json(tmp_path, monkeypatch):
    from pevit_amd.commands import zeroshot as cmd
    from pevit_amd.evaluation import clip_load
    feat, text = _seeded(N=12, Cc=5, seed=7)
    text_dc = text.t().contiguous()
    want = _f64_probs(feat, text_dc)
    labels = want.argmax(1).clone()
    labels[0] = (labels[0] + 1) % 5
    root = tmp_path / "data"; root.mkdir()
    # the reference's file: three arrays back to back (zeroshot.py:43-47 reads them with three np.load calls)
    with open(root / "zeroshot_features_ViT-B32_wiki_False_gpt3_False.npy", "wb") as f:
        np.save(f, feat.numpy()); np.save(f, text_dc.numpy()); np.save(f, labels.numpy())
    model = tmp_path / "model.yaml"
    model.write_text("MODEL:\n  NAME: 'ViT-B/32'\n  SPEC:\n    EMBED_DIM: 64\nTEST:\n  METRIC: 'accuracy'\n")
    ds = tmp_path / "ds.yaml"
    ds.write_text(f"DATASET:\n  DATASET: 'toy-set'\n  ROOT: '{root}'\n  NUM_CLASSES: 5\n")
    monkeypatch.setattr(cmd, "config", default_config())

    def no_model(*a, **k):
        raise AssertionError("the feature-file route must not build a model")
    for loader in ("load", "plain_load", "_load"):
        monkeypatch.setattr(clip_load, loader, no_model)
    result, probs, metric = cmd.main(["--ds", str(ds), "--model", str(model), "OUTPUT_DIR", str(tmp_path / "out")])
    assert metric == "accuracy" and abs(result - 11 / 12) < 1e-12 and max_rel(probs, want) <= 1e-5
    exp = "zeroshot_eval_wiki_False_wnh_False_wnd_False_gpt3_Falseagg_WIKI_AND_GPT3_gpt3count_1"      # zeroshot.py:89-90
    path = tmp_path / "out" / "predictions" / exp / "toy-set.json"
    assert path.is_file()
    text_json = path.read_text()
    j = json.loads(text_json)
    assert set(j) == NINE_KEYS
    assert j["model_name"] == "CLIP-ViT-B/32" and j["dataset_name"] == "toy-set"
    assert j["n_shot"] == 0 and j["num_trainable_params"] == 0 and j["rnd_seeds"] == [0]
    assert j["num_params"] is None and j["num_visual_params"] is None and j["num_backbone_params"] is None
    p = np.asarray(j["predictions"])
    assert p.shape == (1, 12, 5)
    assert np.array_equal(p[0], np.round(probs.double().numpy(), 6))                     # six digits
    assert all(len(tok.split(".")[1]) <= 6 for tok in re.findall(r"\d+\.\d+(?![\de])", text_json))
    with pytest.raises(SystemExit):
        cmd.main(["--model", str(model), "--text_feature_only"])


def test_the_reference_path_alias_resolves_to_the_command():
    alias = importlib.import_module("vision_benchmark.commands.zeroshot")
    from pevit_amd.commands import zeroshot as cmd
    assert alias.main is cmd.main


def test_the_default_config_has_the_keys_the_experiment_name_needs():
    cfg = default_config()
    assert cfg.KNOWLEDGE.AGGREGATION.MEHTOD == "WIKI_AND_GPT3" and cfg.KNOWLEDGE.AGGREGATION.NUM_GPT3_ITEMS == 1
