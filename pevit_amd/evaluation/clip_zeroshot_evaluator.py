"""CLIP zero-shot evaluation (reference: evaluation/clip_zeroshot_evaluator.py:10-22): extracted image features against the
per-class text features, ``softmax(100 * normalize(image_features) @ text_features)``, scored with ``config.TEST.METRIC``.

This is the host form: numpy in, plain torch, runs without a GPU -- what the zero-shot command uses on a feature file.  On the
engine the same arithmetic is one launch behind the tower (``HipEngine.zeroshot``, csrc/zeroshot.hip), which the command uses when
it has to extract the features itself.
"""
import torch
import torch.nn.functional as F

from .metric import get_metric


def clip_zeroshot_evaluator(image_features, text_features, image_labels, config):
    """image_features (N, D), text_features (D, C), image_labels (N,) or multi-hot (N, C), all numpy ->
    (result, probabilities (N, C) tensor, metric name)."""
    metric = get_metric(config.TEST.METRIC)
    image_features = torch.from_numpy(image_features)
    text_features = torch.from_numpy(text_features).to(image_features.dtype)
    image_labels = torch.from_numpy(image_labels)

    image_features = F.normalize(image_features)
    logits = (100. * image_features @ text_features).softmax(dim=-1)
    result = metric(image_labels.squeeze().cpu().detach().numpy(), logits.cpu().detach().numpy())
    return result, logits, metric.__name__
