"""Linear probe with the reference's module surface (evaluation/full_model_finetune.py:71-495 with
``TRAIN.FREEZE_IMAGE_BACKBONE True``): a BatchNorm1d + Linear head over the frozen CLIP image tower.

Nothing below the head trains, the dataset transforms are deterministic and the archives here are tensors, so every image needs
the tower once per checkpoint.  When a loader is this project's ``TensorLoader`` the features of every row it can yield are
encoded once (``HipEngine.encode_image`` in fixed chunks) into a cache shared by the train / val views, the merged train+val
loader, all sweep runs and the final run; a step is then head-only work on 512-wide rows -- ``pevit_probe_step``, two launches
(csrc/probe.hip) -- and a validation is one ``pevit_probe_predict`` call over the whole split.  The epoch's index batches are
those of ``TensorLoader.iter_indices()``, drawn at the same point of the process-wide generator as the uncached loop draws
them.  With a torch ``DataLoader`` or ``TRAIN.CACHE_FEATURES False`` the probe runs uncached through the shared harness
(``fused_train_step`` / ``fused_predict`` on the ``none`` tower).

``FREEZE_IMAGE_BACKBONE False`` is the reference's full fine-tuning: training every weight of the tower is not built here and
is refused.  Implementation shared with the PEFT harnesses in :mod:`._harness`.
"""
from __future__ import annotations

import itertools
import logging
import math
import threading
import time

import torch
import torch.nn.functional as F
from torch import nn

from . import _harness as _h
from ._harness import (MULTILABEL_DATASETS, AverageMeter, accuracy, adjust_learning_rate, clone_loader, gpu_gc,  # noqa: F401
                       merge_trainval_loader)
from .clip_load import *  # noqa: F401,F403
from .dataloader import TensorLoader, _Tensors, _View
from .feature import _engine_feature_chunks, _image_engine
from .metric import get_metric
from ..engine_optim import clip_grad_norm
from ..optim import build_optimizer  # noqa: F401

METHOD = "none"
ENCODE_CHUNK = 128          # images per encode_image call while the cache is filled


def get_cls_model(config, feature_type="image"):
    return _h.get_cls_model(METHOD, config, feature_type)


# ---- the feature cache ---------------------------------------------------------------------------------------------------------------
# The cache is shared by the runs of a concurrent sweep (_harness.run_tasks: worker threads, each under its own stream and its own
# engine).  _LOCK serialises the look-up and every fill, so the second worker waits and finds the rows present; a fill, and the
# cache's own zero-fill, is synchronised on the filling worker's stream BEFORE its rows are marked present, so whichever stream
# reads a present row afterwards reads finished memory.
_LOCK = threading.RLock()


def _stream_sync(device):
    if device.type == "cuda":
        torch.cuda.current_stream(device).synchronize()


class FeatureCache:
    """One f32 feature row per image of ONE ``_Tensors`` set that a run can draw; rows are filled on demand, each once."""

    def __init__(self, full, dim, device):
        self.full, self.device = full, torch.device(device)          # (the set is kept alive: its id is part of the key)
        self.feats = torch.zeros((len(full), dim), dtype=torch.float32, device=self.device)
        self.labels = full.labels.to(self.device)
        _stream_sync(self.device)
        self.have = torch.zeros(len(full), dtype=torch.bool)
        self.encoded = 0

    def ensure(self, rows, encode):
        """Encode the rows of ``rows`` (any integer sequence / tensor of row numbers) that are not cached yet, ascending, in
        chunks of ENCODE_CHUNK; ``encode(row_numbers: LongTensor on the host) -> (n, D)`` features, on this cache's device or
        not.  One caller at a time: a second thread waits for the first one's fill and encodes only what is still missing."""
        rows = torch.as_tensor(rows, dtype=torch.long).cpu().unique()
        with _LOCK:
            missing = rows[~self.have[rows]]
            if missing.numel() == 0:
                return self
            for lo in range(0, missing.numel(), ENCODE_CHUNK):
                sel = missing[lo:lo + ENCODE_CHUNK]
                f = torch.as_tensor(encode(sel)).to(device=self.device, dtype=torch.float32)
                self.feats[sel.to(self.device)] = f
            _stream_sync(self.device)                               # the rows are present only once every stream can read them
            self.have[missing] = True
            self.encoded += int(missing.numel())
        return self


_FEATURES = {}          # (checkpoint, weight format, input normalisation) -> {id(_Tensors set): FeatureCache}, one checkpoint at a time
MAX_CACHED_SETS = 4


def feature_cache(key, full, dim, device):
    """The cache of ``full`` under ``key`` (keyed like _BACKBONES / _ZEROSHOT: another checkpoint, weight format or input
    normalisation drops everything cached before)."""
    with _LOCK:
        if key not in _FEATURES:
            _FEATURES.clear()
            _FEATURES[key] = {}
        sets = _FEATURES[key]
        c = sets.get(id(full))
        if c is None or c.full is not full or c.device != torch.device(device) or c.feats.shape[1] != dim:
            while len(sets) >= MAX_CACHED_SETS:
                sets.pop(next(iter(sets)))
            c = sets[id(full)] = FeatureCache(full, dim, device)
        return c


def clear_feature_cache():
    with _LOCK:
        _FEATURES.clear()


def loader_rows(loader):
    """(the underlying ``_Tensors`` set, the row numbers the loader can yield) of a TensorLoader, else None."""
    if not isinstance(loader, TensorLoader):
        return None
    ds = loader.dataset
    if isinstance(ds, _View) and isinstance(ds.dataset, _Tensors):
        return ds.dataset, torch.as_tensor(ds.indices, dtype=torch.long)
    if isinstance(ds, _Tensors):
        return ds, torch.arange(len(ds))
    return None


def epoch_index_batches(loader):
    """The epoch's index batches: exactly ``TensorLoader.iter_indices()``, its shuffle drawn inside ``ordered_section()`` on the
    way to the first batch, as ``_harness.train_one`` draws it."""
    it = loader.iter_indices()
    with _h.ordered_section():
        first = next(it, None)
    return () if first is None else itertools.chain((first,), it)


# ---- route selection -----------------------------------------------------------------------------------------------------------------
def select_probe_route(criterion, optimizer, *, has_channel_bn=True, bn_momentum=0.1, bn_eps=1e-5, normalize=False,
                       trainable_logit_scale=False, soft_labels=False, layout=None):
    """How one step on cached rows runs.  Pure: no GPU, no engine.
    "fused":    ``pevit_probe_step`` with the SGD update inside its second launch -- torch.optim.SGD with one set of
                hyper-parameters;
    "plan":     ``pevit_probe_step`` without the update, then ``pevit_optim_step`` -- Adam, AdamW, SGD whose groups differ
                (``plan_fused_optimizer`` over ``layout``, the head's (parameter, offset, numel) list);
    "autograd": torch autograd on the gathered cached rows (the cache still saves the tower) -- a trainable logit scale,
                NORMALIZE_VISUAL_FEATURE, no channel_bn, non-default BatchNorm momentum / eps, label smoothing, class weights, soft
                labels, any other criterion or optimizer."""
    if trainable_logit_scale or normalize or not has_channel_bn or bn_momentum != 0.1 or bn_eps != 1e-5 or soft_labels:
        return "autograd"
    if isinstance(criterion, nn.BCEWithLogitsLoss):
        if criterion.weight is not None or criterion.pos_weight is not None or criterion.reduction != "mean":
            return "autograd"
    elif isinstance(criterion, nn.CrossEntropyLoss):
        if criterion.weight is not None or criterion.reduction != "mean" or getattr(criterion, "label_smoothing", 0.0) != 0.0 \
                or criterion.ignore_index != -100:
            return "autograd"
    else:
        return "autograd"
    live = [g for g in optimizer.param_groups if len(g["params"]) > 0]
    if type(optimizer) is torch.optim.SGD and live:
        g0 = live[0]
        same = all((g["lr"], g["momentum"], g["weight_decay"], g["nesterov"]) == (g0["lr"], g0["momentum"], g0["weight_decay"],
                                                                                 g0["nesterov"]) for g in live)
        plain = all(g["dampening"] == 0 and not g.get("maximize", False) for g in live)
        if same and plain:
            return "fused"
    if layout is not None and _h.plan_fused_optimizer(optimizer, layout) is not None:
        return "plan"
    return "autograd"


class Classifier(_h.ClassifierBase):
    """Linear classifier on the frozen tower."""
    METHOD = METHOD

    def __init__(self, config, l2_lambda):
        if not config.TRAIN.FREEZE_IMAGE_BACKBONE:
            raise NotImplementedError("TRAIN.FREEZE_IMAGE_BACKBONE False is full fine-tuning: training the weights of the image "
                                      "tower (a weight-gradient pass through every block) is not built; the linear probe needs "
                                      "TRAIN.FREEZE_IMAGE_BACKBONE True")
        super().__init__(config, l2_lambda)
        for name, param in self.backbone.named_parameters():        # reference :84-95: the text tower, logit_scale and every visual* tensor
            param.requires_grad = False
        self._cache_features = bool(config.TRAIN.get("CACHE_FEATURES", True))
        self._cache_key = (str(config.MODEL.NAME), str(self.backbone.visual.weight_format),
                           getattr(self.backbone.visual, "_input_norm", None))

    def scale(self) -> float:
        return float(math.exp(float(self.logit_scale.detach())))

    def head(self, feature):
        """channel_bn -> [normalize] -> logit_scale.exp() * Linear (reference :146-157) on feature rows"""
        outputs = self.channel_bn(feature)
        if self.normalize_visual_output:
            outputs = F.normalize(outputs)
        return self.logit_scale.exp() * self.layers(outputs)

    def forward(self, img):
        pdtype = torch.float32 if img.dtype == torch.uint8 else img.dtype
        if img.is_cuda:
            self.engine()
        return self.head(self.backbone(img).to(pdtype))

    # the engine's image-to-logits calls have no scale: they are this module's forward only while exp(logit_scale) is exactly 1
    def _fusable_step(self, criterion) -> bool:
        return self.scale() == 1.0 and super()._fusable_step(criterion)

    def can_fuse_eval(self, images=None) -> bool:
        return self.scale() == 1.0 and super().can_fuse_eval(images)

    # ---- cached route ---------------------------------------------------------------------
    def cached(self, loader):
        """The FeatureCache behind ``loader`` with every row the loader can yield encoded, or None (not a TensorLoader,
        TRAIN.CACHE_FEATURES False, the tower not on a GPU)."""
        if not self._cache_features or self.backbone.visual.class_embedding.device.type != "cuda":
            return None
        lr = loader_rows(loader)
        if lr is None:
            return None
        full, rows = lr
        eng = self.engine()
        cache = feature_cache(self._cache_key, full, eng.arch.embed_dim, eng.device)

        def encode(sel):
            chunk = TensorLoader(_View(full, sel.tolist()), batch_size=ENCODE_CHUNK, shuffle=False)
            (f, _), = _engine_feature_chunks(_image_engine(None, self.backbone, chunk), chunk)      # one batch, left on the device
            return f
        start, before = time.time(), cache.encoded
        cache.ensure(rows, encode)
        if cache.encoded != before:
            logging.info(f"=> Feature cache: {cache.encoded - before} rows encoded in {time.time() - start:.2f}s "
                         f"({cache.encoded} of {len(full)} rows of this set cached)")
        return cache

    def probe_route(self, criterion, optimizer, cache):
        bn = self.channel_bn
        has_bn = isinstance(bn, nn.BatchNorm1d)
        soft = isinstance(criterion, nn.CrossEntropyLoss) and cache.labels.is_floating_point()
        if isinstance(criterion, nn.BCEWithLogitsLoss) and not (cache.labels.dim() == 2 and cache.labels.dtype == torch.float32):
            soft = True
        layout = [(self.layers[0].weight, 0, self.layers[0].weight.numel()),
                  (self.layers[0].bias, self.layers[0].weight.numel(), self.layers[0].bias.numel())]
        if {id(p) for p in self.parameters() if p.requires_grad} != {id(p) for p, _, _ in layout}:
            return "autograd", None
        route = select_probe_route(criterion, optimizer, has_channel_bn=has_bn, bn_momentum=bn.momentum if has_bn else None,
                                   bn_eps=bn.eps if has_bn else None, normalize=self.normalize_visual_output,
                                   trainable_logit_scale=self.logit_scale.requires_grad, soft_labels=soft,
                                   layout=layout if self._fused_optimizer else None)
        plan = _h.plan_fused_optimizer(optimizer, layout) if route == "plan" else None
        return route, plan


def train_one(train_loader, model, criterion, optimizer, epoch, config):
    model.train()                                             # reference :299 (the frozen ViT has nothing that depends on the mode)
    cache = model.cached(train_loader)
    if cache is None:
        return _h.train_one(train_loader, model, criterion, optimizer, epoch, config)
    metric = get_metric(config.TEST.METRIC)
    losses = AverageMeter()
    route, plan = model.probe_route(criterion, optimizer, cache)
    eng = model.engine()
    dev = eng.device
    n_total = len(train_loader.dataset)
    out_buf = torch.empty((n_total, config.DATASET.NUM_CLASSES), dtype=torch.float32, device=dev)
    loss_buf = torch.empty((len(train_loader) + 1,), dtype=torch.float32, device=dev)
    picked, sizes = [], []
    row = step = 0
    scale = model.scale()
    # TRAIN.CLIP_GRAD_NORM > 0 (reference :327-328): clip_grad_norm_ between the backward and the step.  On the engine routes the
    # step is then taken apart -- gradients only, the clip (two launches, no host read), the update as its own call
    clip = float(config.TRAIN.get("CLIP_GRAD_NORM", 0.0) or 0.0)
    clip = clip if clip > 0 else None
    try:
        for sel in epoch_index_batches(train_loader):
            n = sel.shape[0]
            if n == 1:
                continue                                      # BatchNorm cannot take a single-sample batch (reference :316)
            sel = sel.to(dev).contiguous()
            logits_out, loss_out = out_buf[row:row + n], loss_buf[step:step + 1]
            if route == "autograd":
                target = cache.labels[sel]
                optimizer.zero_grad()
                output = model.head(cache.feats[sel])
                loss = criterion(output, target)
                loss.backward()
                if clip is not None:
                    torch.nn.utils.clip_grad_norm_(model.parameters(), clip)
                optimizer.step()
                logits_out.copy_(output.detach()); loss_out.copy_(loss.detach().reshape(1))
            else:
                eng.ensure_batch(n)
                g = next(g for g in optimizer.param_groups if len(g["params"]) > 0)
                hyper = dict(lr=g["lr"], momentum=g.get("momentum", 0.0), weight_decay=g["weight_decay"],
                             nesterov=bool(g.get("nesterov", False)))
                eng.probe_step(cache.feats, sel, cache.labels, **hyper,
                               bn_training=model.channel_bn.training, scale=scale, update=route == "fused" and clip is None,
                               logits_out=logits_out, loss_out=loss_out)
                if clip is not None:
                    clip_grad_norm(eng, clip)
                if route == "plan":
                    eng.optimizer_step(plan.refresh(optimizer))
                elif clip is not None:
                    eng.sgd_step(**hyper)
                if model.channel_bn.training:
                    model._bn_steps = getattr(model, "_bn_steps", 0) + 1
            picked.append(sel); sizes.append(n)
            row += n; step += 1
    finally:
        model.flush_bn_counter()
    if not sizes:
        return
    for v, n in zip(loss_buf[:step].cpu().tolist(), sizes):   # one sync per epoch, not per step
        losses.update(v, n)
    metric_result, _ = _h._score(metric, [out_buf[:row]], [cache.labels[torch.cat(picked)]])
    logging.info(f"[Epoch {epoch}] Train: {metric.__name__} {metric_result:.3f}")
    return losses.avg


@torch.no_grad()
def validate(val_loader, model, criterion, epoch, config, return_logits=False):
    cache = model.cached(val_loader)
    if cache is None:
        return _h.validate(val_loader, model, criterion, epoch, config, return_logits=return_logits)
    metric = get_metric(config.TEST.METRIC)
    eng = model.engine()
    eng.check_streamk()
    model.eval()
    _, rows = loader_rows(val_loader)
    rows = rows.to(eng.device)
    bn = model.channel_bn
    if isinstance(bn, nn.BatchNorm1d) and bn.eps == 1e-5 and not model.normalize_visual_output:
        whole = rows.numel() == len(cache.full) and bool((rows == torch.arange(rows.numel(), device=rows.device)).all())
        # one call for the whole split, not one per batch
        output = eng.probe_predict(cache.feats, index=None if whole else rows.contiguous(), scale=model.scale())
    else:
        output = model.head(cache.feats[rows])
    metric_result, logits = _h._score(metric, [output], [cache.labels[rows]])
    logging.info(f"[Epoch {epoch}] Val: {metric.__name__} {metric_result:.3f}")
    return (metric_result, logits) if return_logits else metric_result


def train_task(train_dataloader, test_dataloader, config, sweep_run=False):
    return _h.train_task(Classifier, train_dataloader, test_dataloader, config, sweep_run=sweep_run,
                         train_one_fn=train_one, validate_fn=validate)


def hyperparameter_sweep(train_dataloader, val_dataloader, config):
    return _h.hyperparameter_sweep(train_task, train_dataloader, val_dataloader, config)


def hyperparameter_sweep_lr(train_dataloader, val_dataloader, config):
    return _h.hyperparameter_sweep_lr(hyperparameter_sweep, train_dataloader, val_dataloader, config)


def full_model_finetune(train_dataloader, val_dataloader, test_dataloader, no_hyperparameter_tuning, lr, l2, config):
    return _h.final_run(train_task, hyperparameter_sweep_lr, train_dataloader, val_dataloader, test_dataloader,
                        no_hyperparameter_tuning, lr, l2, config)
