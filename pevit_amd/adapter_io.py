"""Adapter checkpoints: what a fine-tune run produces -- the adapter tensors, the Linear head, the BatchNorm running statistics --
as ONE small file, and the way back into a training ``Classifier`` (``load_adapter``) or into a serving context
(``serving.InferenceEngine.add_adapter``).

The file is one ``torch.save`` of ``{"format": "pevit-adapter", "version": 1, "meta": {...}, "tensors": {...}}`` holding plain
tensors, numbers, strings and lists only; it is read with ``torch.load(..., weights_only=True)`` and nothing else.

``tensors`` (all f32, CPU, contiguous): EVERY entry of ``adapter_param_spec(method, width, layers, lora_rank)``, trainable or not
(Compacter's frozen ``phm_rule`` is drawn at construction and is in no CLIP checkpoint; KAdaptation's dead ``v_proj_adapter1_*``
keep the flat buffer reloadable bit for bit), ``layers.0.weight`` / ``layers.0.bias``, ``channel_bn.running_mean`` /
``running_var`` / ``num_batches_tracked`` and ``logit_scale``.  ``meta``: see ``META_KEYS``.  Optimizer state is not part of a
checkpoint.  Everything here but ``adapter_state`` on a live engine is host-only: no GPU, no engine.
"""
from __future__ import annotations

import hashlib
import math
import os
import pickle
import warnings

import torch

from .engine import adapter_param_spec

FORMAT, VERSION = "pevit-adapter", 1
ARCH_KEYS = ("width", "layers", "patch", "resolution", "embed_dim")
# what every checkpoint's meta holds; "epoch" and "score" join them when the writer knows them
META_KEYS = ("method", "lora_rank", "arch", "num_classes", "weight_format", "input_mean", "input_std", "center_crop", "dataset",
             "metric", "use_channel_bn", "normalize_visual_feature", "trainable_logit_scale", "backbone_sha256")
HEAD_TENSORS = ("layers.0.weight", "layers.0.bias", "channel_bn.running_mean", "channel_bn.running_var",
                "channel_bn.num_batches_tracked", "logit_scale")
FINGERPRINT_KEYS = ("class_embedding", "positional_embedding", "proj")


class AdapterError(ValueError):
    """A checkpoint that is refused; the message starts with the offending field."""


# ---- pieces -------------------------------------------------------------------------------------------------------------------------
def _f32(t):
    return torch.as_tensor(t).detach().to(device="cpu", dtype=torch.float32).contiguous().clone()


def backbone_fingerprint(sd, prefix: str = "visual.") -> str:
    """sha256 over the f32 bytes of ``class_embedding``, ``positional_embedding`` and ``proj`` of a tower (an OpenAI-layout
    state dict, or anything indexable by those names under ``prefix``)."""
    h = hashlib.sha256()
    for k in FINGERPRINT_KEYS:
        h.update(_f32(sd[prefix + k]).numpy().tobytes())
    return h.hexdigest()


def arch_numbers(arch) -> dict:
    """The five numbers of a ``VitArch`` (or of a meta's ``arch`` dict) that fix the tower's shapes."""
    return {k: int(arch[k] if isinstance(arch, dict) else getattr(arch, k)) for k in ARCH_KEYS}


def expected_tensors(meta) -> dict:
    """name -> shape of every tensor a checkpoint with this meta must hold."""
    a, C = meta["arch"], int(meta["num_classes"])
    D = int(a["embed_dim"])
    out = {n: tuple(s) for n, s, _ in adapter_param_spec(meta["method"], int(a["width"]), int(a["layers"]), int(meta["lora_rank"]))}
    out.update({"layers.0.weight": (C, D), "layers.0.bias": (C,), "channel_bn.running_mean": (D,), "channel_bn.running_var": (D,),
                "channel_bn.num_batches_tracked": (), "logit_scale": ()})
    return out


def flat_params(ckpt) -> torch.Tensor:
    """The engine's flat f32 buffer of a checkpoint: the TRAINABLE tower tensors in ``adapter_param_spec`` order, head W, head b."""
    m, t = ckpt["meta"], ckpt["tensors"]
    names = [n for n, _, tr in adapter_param_spec(m["method"], int(m["arch"]["width"]), int(m["arch"]["layers"]), int(m["lora_rank"])) if tr]
    return torch.cat([t[n].reshape(-1) for n in names + ["layers.0.weight", "layers.0.bias"]])


def make_adapter(meta: dict, tensors: dict) -> dict:
    """The checkpoint dict of ``meta`` and ``tensors`` (copied to f32 CPU), checked like a file that was read."""
    ckpt = {"format": FORMAT, "version": VERSION, "meta": dict(meta), "tensors": {k: _f32(v) for k, v in tensors.items()}}
    ckpt["meta"]["arch"] = arch_numbers(meta["arch"])
    return check_adapter(ckpt)


# ---- checks -------------------------------------------------------------------------------------------------------------------------
def check_adapter(ckpt, *, method=None, lora_rank=None, arch=None, num_classes=None, max_classes=None, backbone_sha256=None,
                  strict_backbone: bool = True) -> dict:
    """Refuse (``AdapterError``, the message names the field) a checkpoint of the wrong format or version, with a missing,
    extra or mis-shaped tensor or a non-finite value -- and, where the caller says what it holds, of another method, LoRA rank,
    arch or class count (``num_classes``: exactly; ``max_classes``: at most) or trained on another backbone
    (``strict_backbone=False``: a warning).  Returns ``ckpt``."""
    if not isinstance(ckpt, dict) or ckpt.get("format") != FORMAT:
        raise AdapterError(f"format: expected {FORMAT!r}, got {ckpt.get('format') if isinstance(ckpt, dict) else type(ckpt).__name__!r}")
    if ckpt.get("version") != VERSION:
        raise AdapterError(f"version: this build reads version {VERSION}, the checkpoint has {ckpt.get('version')!r}")
    meta, tensors = ckpt.get("meta"), ckpt.get("tensors")
    if not isinstance(meta, dict) or not isinstance(tensors, dict):
        raise AdapterError("format: 'meta' and 'tensors' must be dicts")
    for k in META_KEYS:
        if k not in meta:
            raise AdapterError(f"meta.{k}: missing")
    if not isinstance(meta["arch"], dict) or any(k not in meta["arch"] for k in ARCH_KEYS):
        raise AdapterError(f"meta.arch: expected the numbers {ARCH_KEYS}")
    try:
        want = expected_tensors(meta)
    except (ValueError, TypeError) as e:
        raise AdapterError(f"method: {e}") from None
    for name, shape in want.items():
        if name not in tensors:
            raise AdapterError(f"tensor {name}: missing")
        t = tensors[name]
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.device.type != "cpu" or not t.is_contiguous():
            raise AdapterError(f"tensor {name}: must be a contiguous float32 CPU tensor")
        if tuple(t.shape) != shape:
            raise AdapterError(f"tensor {name}: shape {tuple(t.shape)}, expected {shape}")
        if not bool(torch.isfinite(t).all()):
            raise AdapterError(f"tensor {name}: non-finite value")
    for name in tensors:
        if name not in want:
            raise AdapterError(f"tensor {name}: not part of a {meta['method']} checkpoint")
    # ---- against what the caller holds
    if method is not None and meta["method"] != method:
        raise AdapterError(f"method: the checkpoint is {meta['method']!r}, expected {method!r}")
    if lora_rank is not None and meta["method"] == "lora" and int(meta["lora_rank"]) != int(lora_rank):
        raise AdapterError(f"lora_rank: the checkpoint has {meta['lora_rank']}, expected {lora_rank}")
    if arch is not None:
        have, exp = arch_numbers(meta["arch"]), arch_numbers(arch)
        for k in ARCH_KEYS:
            if have[k] != exp[k]:
                raise AdapterError(f"arch.{k}: the checkpoint has {have[k]}, expected {exp[k]}")
    if num_classes is not None and int(meta["num_classes"]) != int(num_classes):
        raise AdapterError(f"num_classes: the checkpoint has {meta['num_classes']}, expected {num_classes}")
    if max_classes is not None and not 1 <= int(meta["num_classes"]) <= int(max_classes):
        raise AdapterError(f"num_classes: the checkpoint has {meta['num_classes']}, the context serves 1 to {max_classes}")
    if backbone_sha256 is not None and meta["backbone_sha256"] != backbone_sha256:
        msg = (f"backbone_sha256: the checkpoint was trained on tower {str(meta['backbone_sha256'])[:12]}..., the loaded tower is "
               f"{backbone_sha256[:12]}...")
        if strict_backbone:
            raise AdapterError(msg + " (strict_backbone=False loads it anyway)")
        warnings.warn(msg)
    return ckpt


def check_servable(ckpt) -> dict:
    """What ``pevit_predict`` computes is tower -> BatchNorm1d(affine=False) in eval mode -> Linear: refuse the head switches it
    does not compute -- no channel BN, normalised features, and for the linear probe (method ``none``, whose forward multiplies
    by ``exp(logit_scale)``; the adapter classifiers never apply theirs) a scale other than 1."""
    meta = ckpt["meta"]
    if not meta["use_channel_bn"]:
        raise AdapterError("use_channel_bn: False -- the engine's predict always runs the BatchNorm1d of the head")
    if meta["normalize_visual_feature"]:
        raise AdapterError("normalize_visual_feature: True -- the engine's predict does not normalise the features")
    if meta["method"] == "none" and math.exp(float(ckpt["tensors"]["logit_scale"])) != 1.0:
        raise AdapterError(f"logit_scale: exp({float(ckpt['tensors']['logit_scale'])}) is not 1 -- the engine's predict has no logit scale")
    return ckpt


# ---- files --------------------------------------------------------------------------------------------------------------------------
def write_adapter(ckpt: dict, path) -> str:
    """``torch.save`` of a checked checkpoint dict; the folder is created."""
    check_adapter(ckpt)
    folder = os.path.dirname(os.path.abspath(os.fspath(path)))
    os.makedirs(folder, exist_ok=True)
    torch.save(ckpt, os.fspath(path))
    return os.fspath(path)


def read_adapter(path) -> dict:
    """Read and check a checkpoint file.  Only what ``torch.load(weights_only=True)`` accepts is read: a file that needs
    unpickling of anything but tensors and plain containers is refused."""
    try:
        ckpt = torch.load(os.fspath(path), map_location="cpu", weights_only=True)
    except (pickle.UnpicklingError, RuntimeError, AttributeError, TypeError) as e:
        raise AdapterError(f"format: {os.fspath(path)} is not a tensors-only adapter checkpoint ({str(e).splitlines()[0]})") from None
    return check_adapter(ckpt)


def _as_ckpt(ckpt):
    return read_adapter(ckpt) if isinstance(ckpt, (str, os.PathLike)) else ckpt


# ---- a training Classifier ----------------------------------------------------------------------------------------------------------
def _proj_merged(visual) -> bool:
    p = visual.proj.detach()
    return p.shape[0] == p.shape[1] and bool(torch.equal(p, torch.eye(p.shape[0], dtype=p.dtype, device=p.device)))


def refuse_merged(classifier, what):
    if _proj_merged(classifier.backbone.visual):
        raise AdapterError(f"merge_encoder_and_head_proj: {what} a TRAIN.MERGE_ENCODER_AND_HEAD_PROJ classifier is not supported -- "
                           "its tower no longer owns visual.proj (the head holds it), and the reference's scripts pass False")


def config_meta(config) -> dict:
    """The meta entries that come from the run's config: input normalisation, crop mode, dataset name and metric."""
    ds = config.DATASET
    crop = ds.get("CENTER_CROP", True) if hasattr(ds, "get") else getattr(ds, "CENTER_CROP", True)
    return {"input_mean": [float(v) for v in config.INPUT.MEAN], "input_std": [float(v) for v in config.INPUT.STD],
            "center_crop": bool(crop), "dataset": str(ds.DATASET), "metric": str(config.TEST.METRIC)}


def adapter_state(classifier, **extra_meta) -> dict:
    """The checkpoint dict of a ``Classifier`` of the fine-tune harness, as a CPU copy (a few MB at most).  A pending pipelined DP
    step and the BatchNorm counter are flushed first.  ``extra_meta`` (``config_meta(config)``, ``epoch``, ``score``, ...)
    overrides the defaults."""
    refuse_merged(classifier, "saving")
    visual = classifier.backbone.visual
    if visual._engine is not None:
        visual._engine.dp_flush()
    classifier.flush_bn_counter()
    named = dict(visual.named_parameters())
    spec = adapter_param_spec(visual.method, visual.arch.width, visual.arch.layers, visual.lora_rank)
    tensors = {n: named[n[len("visual."):]] for n, _, _ in spec}
    lin, bn = classifier.layers[0], classifier.channel_bn
    has_bn = isinstance(bn, torch.nn.BatchNorm1d)
    D = lin.weight.shape[1]
    tensors.update({"layers.0.weight": lin.weight, "layers.0.bias": lin.bias,
                    "channel_bn.running_mean": bn.running_mean if has_bn else torch.zeros(D),
                    "channel_bn.running_var": bn.running_var if has_bn else torch.ones(D),
                    "channel_bn.num_batches_tracked": bn.num_batches_tracked if has_bn else torch.zeros(()),
                    "logit_scale": classifier.logit_scale})
    norm = visual._input_norm or ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
    meta = {"method": visual.method, "lora_rank": int(visual.lora_rank), "arch": arch_numbers(visual.arch),
            "num_classes": int(lin.weight.shape[0]), "weight_format": str(visual.weight_format),
            "input_mean": [float(v) for v in norm[0]], "input_std": [float(v) for v in norm[1]],
            "center_crop": bool(visual._resize_center_crop), "dataset": "", "metric": "",
            "use_channel_bn": has_bn, "normalize_visual_feature": bool(classifier.normalize_visual_output),
            "trainable_logit_scale": bool(classifier.logit_scale.requires_grad),
            "backbone_sha256": backbone_fingerprint(named, prefix="")}
    meta.update(extra_meta)
    return make_adapter(meta, tensors)


def engine_adapter_state(eng, backbone_sd, phm_rule=None, prefix: str = "visual.", **extra_meta) -> dict:
    """The checkpoint dict of a bare ``HipEngine`` (no ``Classifier`` around it): its flat buffer and running statistics, the
    fingerprint of ``backbone_sd`` -- the state dict the engine was loaded from, which also holds Compacter's frozen rule unless
    ``phm_rule`` gives it."""
    views = {k: v for k, v in eng.param_views().items()}
    tensors = {}
    for n, s, tr in adapter_param_spec(eng.method, eng.arch.width, eng.arch.layers, eng.lora_rank):
        tensors[n] = views[n] if tr else (phm_rule if phm_rule is not None else backbone_sd[n]).reshape(s)
    tensors.update({"layers.0.weight": views["layers.0.weight"], "layers.0.bias": views["layers.0.bias"],
                    "channel_bn.running_mean": eng.running_mean, "channel_bn.running_var": eng.running_var,
                    "channel_bn.num_batches_tracked": torch.zeros(()), "logit_scale": torch.zeros(())})
    norm = eng._input_norm or ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
    meta = {"method": eng.method, "lora_rank": int(eng.lora_rank), "arch": arch_numbers(eng.arch), "num_classes": int(eng.num_classes),
            "weight_format": str(eng.weight_format), "input_mean": [float(v) for v in norm[0]], "input_std": [float(v) for v in norm[1]],
            "center_crop": bool(eng._resize_center_crop), "dataset": "", "metric": "", "use_channel_bn": True,
            "normalize_visual_feature": False, "trainable_logit_scale": False,
            "backbone_sha256": backbone_fingerprint(backbone_sd, prefix)}
    meta.update(extra_meta)
    return make_adapter(meta, tensors)


def save_adapter(classifier, path, **extra_meta) -> str:
    """``adapter_state(classifier, **extra_meta)`` written to ``path``."""
    return write_adapter(adapter_state(classifier, **extra_meta), path)


def load_adapter(classifier, ckpt, strict_backbone: bool = True):
    """Put a checkpoint (a path, or the dict ``read_adapter`` returns) back into a training ``Classifier`` of the same method,
    arch and class count, so that a run can continue: the adapter and head tensors through the engine's ``load_trainable`` (or
    straight into the module while it has no engine), the BatchNorm buffers and ``logit_scale`` into the module.  The optimizer
    starts fresh."""
    refuse_merged(classifier, "loading into")
    ckpt = _as_ckpt(ckpt)
    visual = classifier.backbone.visual
    named = dict(visual.named_parameters())
    lin, bn = classifier.layers[0], classifier.channel_bn
    check_adapter(ckpt, method=visual.method, lora_rank=visual.lora_rank, arch=visual.arch, num_classes=lin.weight.shape[0],
                  backbone_sha256=backbone_fingerprint(named, prefix=""), strict_backbone=strict_backbone)
    has_bn = isinstance(bn, torch.nn.BatchNorm1d)
    if bool(ckpt["meta"]["use_channel_bn"]) != has_bn:
        raise AdapterError(f"use_channel_bn: the checkpoint has {ckpt['meta']['use_channel_bn']}, the classifier {has_bn}")
    t = ckpt["tensors"]
    on_gpu = visual.class_embedding.device.type == "cuda"
    eng = classifier.engine() if on_gpu else None          # (binding seats the head and the BatchNorm buffers in the engine)
    with torch.no_grad():
        for n, _, tr in adapter_param_spec(visual.method, visual.arch.width, visual.arch.layers, visual.lora_rank):
            if not tr or eng is None:
                p = named[n[len("visual."):]]
                p.copy_(t[n].to(p.device).view_as(p))
                if not tr and eng is not None and n.endswith("transformer.phm_rule"):
                    eng.load_phm_rule(p)
        if eng is not None:
            eng.load_trainable(t)
        else:
            lin.weight.copy_(t["layers.0.weight"]); lin.bias.copy_(t["layers.0.bias"])
        if has_bn:
            bn.running_mean.copy_(t["channel_bn.running_mean"]); bn.running_var.copy_(t["channel_bn.running_var"])
            bn.num_batches_tracked.copy_(t["channel_bn.num_batches_tracked"].to(torch.int64))
        classifier.logit_scale.copy_(t["logit_scale"])
    classifier._bn_steps = 0
    return classifier
