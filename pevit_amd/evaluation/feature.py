"""Zero-shot head initialisation and loader helpers (reference: evaluation/feature.py:405-531,585-608).

Only what ``Classifier(INIT_HEAD_WITH_TEXT_ENCODER=True)`` needs is here: prompts per class -> text tower
(host PyTorch, one call per class; with ``TRAIN.TEXT_TOWER_ENGINE`` the HIP engine's text tower, all prompts
in chunks) -> normalise / mean over templates / normalise -> (D, C) weight matrix.  The
reference's class-name tables, prompt templates, tokenizer vocabulary and knowledge sources are data of
its dataset layer and are not shipped: the caller supplies them through ``config.DATASET.CLASS_NAMES`` /
``config.DATASET.TEMPLATES`` (or the keyword arguments) and a ``tokenizer(texts, context_length=...)``.
"""
from __future__ import annotations

import logging
import time

import torch


def reduce_class_features(features, class_index, num_classes):
    """The reference's per-class reduction (feature.py:513-520) over a stacked tensor: features (S, D), class_index (S,) int64
    with the class of every row -> (D, C): normalise every row, mean over the rows of a class, normalise."""
    e = features / features.norm(dim=-1, keepdim=True)
    idx = class_index.to(device=e.device, dtype=torch.int64)
    sums = torch.zeros((num_classes, e.shape[1]), dtype=e.dtype, device=e.device).index_add_(0, idx, e)
    counts = torch.bincount(idx, minlength=num_classes).to(e.dtype)
    if bool((counts == 0).any()):
        raise RuntimeError("reduce_class_features: a class without prompts")
    m = sums / counts[:, None]
    return (m / m.norm(dim=-1, keepdim=True)).t().contiguous()


def _class_tokens(config, tokenizer, classname, templates, device):
    """token ids (T, context) of one class's prompts, or the formatted prompts themselves with MODEL.SPEC.TEXT.SKIP_TOKENIZE"""
    if type(classname) == list:
        classname = classname[0]
    if torch.is_tensor(classname):                    # already tokenised prompts of this class: (T, context)
        return classname.to(device)
    texts = [t.format(classname) for t in templates]
    if not config.MODEL.SPEC.TEXT.get("SKIP_TOKENIZE", False):
        if tokenizer is None:
            raise RuntimeError("a tokenizer callable is required to turn prompts into token ids")
        texts = tokenizer(texts, context_length=config.MODEL.SPEC.TEXT.CONTEXT_LENGTH).to(device)
    return texts


@torch.no_grad()
def extract_text_features(config, tokenizer, args=None, model=None, return_numpy=True, class_names=None, templates=None):
    if model is None:
        raise RuntimeError("extract_text_features needs the CLIP model whose text tower is to be used")
    class_names = class_names or config.DATASET.get("CLASS_NAMES", None)
    if not class_names:
        raise RuntimeError("no class names: set config.DATASET.CLASS_NAMES (the reference's class_map / dataset-hub "
                           "lookup, feature.py:408-415, belongs to its dataset layer)")
    templates = templates or config.DATASET.get("TEMPLATES", None) or ["a photo of a {}"]
    know = config.get("KNOWLEDGE", None)
    if know is not None and (know.WIKITIONARY.USE_DEFINITION or know.WORDNET.USE_DEFINITION or know.WORDNET.USE_HIERARCHY
                             or know.GPT3.USE_GPT3):
        raise RuntimeError("knowledge-augmented prompts (KNOWLEDGE.*) are not part of this build")
    device = next(model.parameters()).device
    start = time.time()
    model.eval()
    from ..text_engine import text_engine_ok
    train_cfg = config.get("TRAIN", None) if hasattr(config, "get") else getattr(config, "TRAIN", None)
    engine = bool(train_cfg is not None and train_cfg.get("TEXT_TOWER_ENGINE", False)) and hasattr(model, "encode_text_engine") \
        and text_engine_ok(model)
    if engine:
        # every class tokenised, the prompts stacked into one (S, context) tensor with the class of every row, encoded in chunks
        per_class = [_class_tokens(config, tokenizer, c, templates, device) for c in class_names]
        engine = all(torch.is_tensor(t) for t in per_class)           # (SKIP_TOKENIZE hands strings to encode_text: torch route)
    if engine:
        tokens = torch.cat(per_class, dim=0)
        index = torch.cat([torch.full((t.shape[0],), i, dtype=torch.int64) for i, t in enumerate(per_class)]).to(device)
        try:
            feats = model.encode_text_engine(tokens).to(model.text_projection.dtype)
            zeroshot_weights = reduce_class_features(feats, index, len(per_class)).to(device)
        finally:
            model.release_text_engine()       # its arena must not stay allocated next to the training contexts
    else:
        cols = []
        for classname in class_names:
            texts = _class_tokens(config, tokenizer, classname, templates, device)
            emb = model.encode_text(texts)
            emb = emb / emb.norm(dim=-1, keepdim=True)
            emb = emb.mean(dim=0)
            cols.append(emb / emb.norm())
        zeroshot_weights = torch.stack(cols, dim=1).to(device)
    logging.info(f"=> Feature extraction duration time: {time.time() - start:.2f}s "
                 f"(text tower: {'HIP engine, %d prompts in chunks' % tokens.shape[0] if engine else 'torch, one call per class'})")
    return zeroshot_weights.cpu().detach().numpy() if return_numpy else zeroshot_weights


def _image_engine(config, model, loader):
    """The HIP context of ``model.visual``, sized for the loader's batches and told the preprocessing constants of uint8 sets."""
    visual = model.visual
    if getattr(visual, "_input_norm", None) is None and hasattr(config, "INPUT") and getattr(config.INPUT, "MEAN", None) is not None:
        visual.set_input_normalization(config.INPUT.MEAN, config.INPUT.STD)
        crop = bool(config.DATASET.get("CENTER_CROP", True)) if hasattr(config, "DATASET") and hasattr(config.DATASET, "get") else True
        visual.set_input_resize(True, crop)            # native-size and ragged uint8 sets: Resize + CenterCrop (or squash) in the engine
    eng = visual.engine()
    eng.ensure_batch(int(loader.batch_size))
    return eng


def _engine_feature_chunks(eng, loader):
    """(features (n, D) on the engine's device, labels as the loader yields them) per batch of ``loader``; no synchronise."""
    for x, y in loader:
        yield eng.encode_image(x.to(eng.device, non_blocking=True)), y


def _engine_features(eng, loader):
    feats, labels = zip(*_engine_feature_chunks(eng, loader))
    return torch.cat(feats).cpu().numpy(), torch.cat(labels).cpu().numpy()


@torch.no_grad()
def extract_features(config, model=None, test_split_only=True):
    """Image features of the dataset's splits through ``HipEngine.encode_image`` (reference: feature.py:329-376, which builds the
    model itself; here the caller hands the CLIP model in).  ``test_split_only``: (features (N, D), labels) of the test loader as
    numpy; otherwise the six arrays train / val / test of the reference."""
    from .dataloader import construct_dataloader
    if model is None:
        raise RuntimeError("extract_features needs the CLIP model whose image tower is to be used")
    if test_split_only:
        test = construct_dataloader(config, test_split_only=True)
        return _engine_features(_image_engine(config, model, test), test)
    out = []
    for loader in construct_dataloader(config):
        out += list(_engine_features(_image_engine(config, model, loader), loader))
    return tuple(out)


@torch.no_grad()
def zeroshot_scores(config, model, loader, text_features):
    """The fused zero-shot route: ONE ``HipEngine.zeroshot`` call per batch of ``loader`` (tower + cosine head + softmax).
    text_features: (D, C) as ``extract_text_features`` returns them (numpy or tensor).  Returns (probabilities (N, C), features
    (N, D), labels) as numpy."""
    eng = _image_engine(config, model, loader)
    text_cd = torch.as_tensor(text_features).to(device=eng.device, dtype=torch.float32).t().contiguous()    # class-major, once
    probs, feats, labels = [], [], []
    for x, y in loader:
        p, f = eng.zeroshot(x.to(eng.device, non_blocking=True), text_cd, scale=100.0, return_features=True)
        probs.append(p); feats.append(f); labels.append(y)
    return torch.cat(probs).cpu().numpy(), torch.cat(feats).cpu().numpy(), torch.cat(labels).cpu().numpy()


def create_dataloader(dataset, batch_size, shuffle=True, num_workers=6, pin_memory=True):
    """feature.py:585-608: a plain DataLoader without sampler / drop_last."""
    return torch.utils.data.DataLoader(dataset, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers,
                                       pin_memory=pin_memory, sampler=None, drop_last=False)
