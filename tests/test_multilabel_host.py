"""Multi-label datasets on the host: multi-hot archives in the loader (the greedy validation split of feature.py:150-163,
few-shot selection), the fused-step eligibility of BCEWithLogitsLoss, and the BCE entries of the C ABI."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

from pevit_amd import _lib
from pevit_amd.config import default_config
from pevit_amd.evaluation.dataloader import class_balanced_split, construct_dataloader, few_shot_subset

BCE_ENTRIES = ["pevit_head_forward_backward_bce", "pevit_train_forward_backward_bce", "pevit_train_forward_backward_bce_u8"]

# rows 0..7, classes 0..2; column sums 4, 3, 4
HAND = np.array([[0, 1, 0],
                 [1, 0, 1],
                 [1, 1, 0],
                 [0, 0, 1],
                 [1, 0, 0],
                 [0, 1, 1],
                 [1, 0, 0],
                 [0, 0, 1]], dtype=np.uint8)


def test_greedy_split_of_a_hand_worked_matrix():
    # 0.2: count = ceil(0.8, 0.6, 0.8) = (1, 1, 1).  Class 0 takes row 1 (1,0,1) -> count (0, 1, 0); class 1 takes row 0 -> (0, 0, 0)
    train, val = class_balanced_split(HAND, 0.2)
    assert val == [0, 1] and train == [2, 3, 4, 5, 6, 7]
    # 0.5: count = (2, 2, 2).  Class 0: row 1 -> (1, 2, 1), row 2 -> (0, 1, 1); class 1: row 0 -> (0, 0, 1); class 2: row 3 -> (0, 0, 0)
    train, val = class_balanced_split(HAND, 0.5)
    assert val == [0, 1, 2, 3] and train == [4, 5, 6, 7]
    # a row that pays for two classes: row 1 (0,1,1) is taken for class 1 and brings class 2's count to 0 as well
    y = np.array([[1, 0, 0], [0, 1, 1], [0, 0, 1], [0, 1, 0]], dtype=bool)
    assert class_balanced_split(y, 0.5) == ([2, 3], [0, 1])
    # the same rule for float and bool archives
    assert class_balanced_split(HAND.astype(np.float32), 0.2) == class_balanced_split(HAND.astype(bool), 0.2)


def _multihot(n, c, seed):
    rng = np.random.default_rng(seed)
    y = (rng.random((n, c)) < 0.15).astype(np.uint8)
    y[np.arange(n), rng.integers(0, c, n)] = 1                 # every image has at least one class
    return y


def test_few_shot_on_multi_hot_labels():
    y = _multihot(300, 20, seed=4)
    y[7] = 0                                                  # an image without a positive class is never kept
    keep = few_shot_subset(y, 3, seed=0)
    assert np.array_equal(keep, np.sort(keep)) and len(np.unique(keep)) == len(keep)
    assert 7 not in keep.tolist()
    assert (y[keep].sum(axis=0) >= 3).all()                    # every class reaches its minimum (each has >= 3 samples here)
    assert np.array_equal(keep, few_shot_subset(y, 3, seed=0))
    assert not np.array_equal(keep, few_shot_subset(y, 3, seed=1))
    # a sample is kept only while one of its classes is short: each kept sample fills one of the 3 x 20 places
    assert len(keep) <= 3 * 20


def _voc_config(root, resident=True, shots=0):
    cfg = default_config()
    cfg.merge_from_list(["DATASET.DATASET", "voc-2007-classification", "DATASET.NUM_CLASSES", "20", "TEST.METRIC", "11point_mAP",
                         "DATASET.ROOT", str(root)])
    cfg.DATASET.NUM_SAMPLES_PER_CLASS = shots
    cfg.DATASET.RESIDENT = resident
    return cfg


@pytest.mark.parametrize("resident", [True, False])
def test_loader_reads_multi_hot_archives(tmp_path, resident):
    rng = np.random.default_rng(0)
    ytr, yte = _multihot(90, 20, seed=1), _multihot(12, 20, seed=2)
    np.savez(tmp_path / "voc-2007-classification.npz", train_images=rng.integers(0, 255, (90, 3, 8, 8), dtype=np.uint8),
             train_labels=ytr, test_images=rng.integers(0, 255, (12, 3, 8, 8), dtype=np.uint8), test_labels=yte)
    train, val, test = construct_dataloader(_voc_config(tmp_path, resident))
    full = train.dataset.dataset
    assert full.labels.dtype == torch.float32 and tuple(full.labels.shape) == (90, 20)
    assert np.array_equal(full.labels.cpu().numpy(), ytr.astype(np.float32))
    tr, va = list(train.dataset.indices), list(val.dataset.indices)
    assert sorted(tr + va) == list(range(90)) and not set(tr) & set(va)
    assert (tr, va) == class_balanced_split(ytr, 0.2)
    assert len(test.dataset) == 12
    # the plain fetch and the staging fetch of the DeviceFeeder hand out (B, C) float32 targets
    x, y = next(iter(val))
    assert y.dtype == torch.float32 and tuple(y.shape) == (len(va), 20) and x.dtype == torch.uint8
    assert np.array_equal(y.cpu().numpy(), ytr[va].astype(np.float32))
    (ishape, idt), (tshape, tdt), _ = train.sample_spec()
    assert tshape == (20,) and tdt == torch.float32
    sel = next(train.iter_indices())
    oi = torch.empty((64,) + ishape, dtype=idt, device=sel.device)
    ot = torch.empty((64,) + tshape, dtype=tdt, device=sel.device)
    xi, yt = train.fetch(sel, oi, ot)
    assert yt.dtype == torch.float32 and tuple(yt.shape) == (sel.shape[0], 20)
    assert np.array_equal(yt.cpu().numpy(), ytr[sel.cpu().numpy()].astype(np.float32))
    xt, yt2 = next(iter(test))
    assert yt2.dtype == torch.float32 and tuple(yt2.shape) == (12, 20)


@pytest.mark.parametrize("form", [np.bool_, np.int64, np.float64])
def test_loader_accepts_bool_integer_and_float_archives(tmp_path, form):
    rng = np.random.default_rng(3)
    ytr = _multihot(40, 20, seed=5)
    np.savez(tmp_path / "voc-2007-classification.npz", train_images=rng.standard_normal((40, 3, 8, 8)).astype(np.float32),
             train_labels=ytr.astype(form), test_images=rng.standard_normal((4, 3, 8, 8)).astype(np.float32),
             test_labels=_multihot(4, 20, seed=6).astype(form))
    train, val, _ = construct_dataloader(_voc_config(tmp_path, shots=2))
    full = train.dataset.dataset
    assert full.labels.dtype == torch.float32 and full.labels.shape[1] == 20
    kept = few_shot_subset(ytr.astype(form), 2, seed=int(_voc_config(tmp_path).DATASET.RANDOM_SEED_SAMPLING))
    assert np.array_equal(full.labels.cpu().numpy(), ytr[kept].astype(np.float32))
    assert (full.labels.sum(0) >= 2).all()


def test_single_label_archives_are_unchanged(tmp_path):
    rng = np.random.default_rng(0)
    np.savez(tmp_path / "toy.npz", train_images=rng.standard_normal((20, 3, 8, 8)).astype(np.float32),
             train_labels=(np.arange(20) % 4).astype(np.int32), test_images=rng.standard_normal((4, 3, 8, 8)).astype(np.float32),
             test_labels=(np.arange(4) % 4).reshape(4, 1))
    cfg = default_config()
    cfg.DATASET.DATASET, cfg.DATASET.ROOT, cfg.DATASET.NUM_CLASSES = "toy", str(tmp_path), 4
    train, val, test = construct_dataloader(cfg)
    assert train.dataset.dataset.labels.dtype == torch.int64 and train.dataset.dataset.labels.dim() == 1
    y = test.dataset.labels                                   # (N, 1) stays int64 (N, 1): train_one squeezes it
    assert y.dtype == torch.int64 and tuple(y.shape) == (4, 1)


def _classifier(tmp_path):
    from conftest import load_tiny_sd
    from pevit_amd.evaluation.kadaptation_clip import Classifier
    path = tmp_path / "tiny.pt"
    torch.save(load_tiny_sd(), path)
    cfg = default_config()
    cfg.MODEL.NAME = str(path)
    cfg.MODEL.SPEC.EMBED_DIM = 64
    cfg.MODEL.SPEC.TEXT.CONTEXT_LENGTH = 8
    cfg.DATASET.NUM_CLASSES = 20
    cfg.TRAIN.NESTEROV = False
    cfg.TRAIN.LR, cfg.TRAIN.WD = 0.1, 1e-3
    return cfg, Classifier(cfg, 0)


def test_can_fuse_takes_plain_bce(tmp_path):
    from pevit_amd.optim import build_optimizer
    cfg, clf = _classifier(tmp_path)
    opt = build_optimizer(cfg, clf)
    assert clf.can_fuse(torch.nn.BCEWithLogitsLoss(), opt)
    cfg.TRAIN.NESTEROV = True
    assert clf.can_fuse(torch.nn.BCEWithLogitsLoss(), build_optimizer(cfg, clf))
    cfg.TRAIN.NESTEROV = False
    assert not clf.can_fuse(torch.nn.BCEWithLogitsLoss(weight=torch.ones(20)), opt)
    assert not clf.can_fuse(torch.nn.BCEWithLogitsLoss(pos_weight=torch.ones(20)), opt)
    assert not clf.can_fuse(torch.nn.BCEWithLogitsLoss(reduction="sum"), opt)
    assert not clf.can_fuse(torch.nn.BCEWithLogitsLoss(reduction="none"), opt)
    cfg.TRAIN.WITHOUT_WD_LIST = ["bias"]                      # two weight decays: still the autograd route
    assert not clf.can_fuse(torch.nn.BCEWithLogitsLoss(), build_optimizer(cfg, clf))
    cfg.TRAIN.WITHOUT_WD_LIST = []
    cfg.TRAIN.OPTIMIZER = "adam"
    assert not clf.can_fuse(torch.nn.BCEWithLogitsLoss(), build_optimizer(cfg, clf))
    assert clf.can_fuse(torch.nn.CrossEntropyLoss(), opt)     # the cross-entropy rule is untouched


def test_bce_entries_are_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "pevit_hip.h")).read()
    for name in BCE_ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        res, args = _lib.SIGNATURES[name]
        cross = _lib.SIGNATURES[name.replace("_bce", "")]
        assert (res, args) == cross                           # the same arguments as the CE entry, targets in place of labels
