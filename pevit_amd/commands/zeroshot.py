"""python -m pevit_amd.commands.zeroshot --ds <dataset.yaml> --model <model.yaml> [--save-predictions] [KEY VALUE ...]
(reference: commands/zeroshot.py): zero-shot evaluation of plain CLIP, the ``n_shot: 0`` row every few-shot result is compared with.

Same flags, same config layering (dataset yaml <- model yaml <- KEY VALUE opts), same output file
``<OUTPUT_DIR>/predictions/<exp_name>/<dataset>.json`` with the reference's nine keys.  If the reference's feature file
``<DATASET.ROOT>/zeroshot_features_<name>_wiki_<..>_gpt3_<..>.npy`` exists (three arrays back to back: image features, text
features (D, C), labels) it is loaded and scored on the host with ``clip_zeroshot_evaluator`` -- no GPU needed.  Otherwise the model
is built without adapters (engine method ``none``), the text features come from ``extract_text_features`` (the caller supplies
class names, templates and a tokenizer; ``TRAIN.TEXT_TOWER_ENGINE`` runs the prompts on the engine's text tower) and every test
batch is scored by ONE ``HipEngine.zeroshot`` call: tower, cosine head and softmax.
"""
from __future__ import annotations

import argparse
import logging
import os

import numpy as np
import torch

from ..config import config, update_config
from ..evaluation.clip_zeroshot_evaluator import clip_zeroshot_evaluator
from ..evaluation.metric import get_metric
from ._finetune import json_prec_dump


def add_zero_shot_args(parser):
    parser.add_argument("--ds", required=False, help="Evaluation dataset configure file name.", type=str)
    parser.add_argument("--model", required=True, help="Clip model configure file name", type=str)
    parser.add_argument("--text_feature_only", help="consider text feature or not.", default=False, action="store_true")
    parser.add_argument("--save-predictions", help="save predictions logits for analysis.", default=True, action="store_true")
    parser.add_argument("opts", help="Modify config options using the command-line", default=None, nargs=argparse.REMAINDER)


def feature_file_path(cfg):
    """zeroshot.py:40 of the reference"""
    return os.path.join(cfg.DATASET.ROOT, "zeroshot_features_" + cfg.MODEL.NAME.replace("/", "") +
                        f"_wiki_{cfg.KNOWLEDGE.WIKITIONARY.USE_DEFINITION}" + f"_gpt3_{cfg.KNOWLEDGE.GPT3.USE_GPT3}" + ".npy")


def experiment_name(cfg):
    """zeroshot.py:89-90 of the reference (KNOWLEDGE.AGGREGATION.MEHTOD is its spelling)"""
    k = cfg.KNOWLEDGE
    return ("zeroshot_eval_" + f"wiki_{k.WIKITIONARY.USE_DEFINITION}_wnh_{k.WORDNET.USE_HIERARCHY}_wnd_{k.WORDNET.USE_DEFINITION}"
            f"_gpt3_{k.GPT3.USE_GPT3}" + f"agg_{k.AGGREGATION.MEHTOD}_gpt3count_{k.AGGREGATION.NUM_GPT3_ITEMS}")


def score_on_engine(cfg, tokenizer=None, class_names=None):
    """Build plain CLIP, text features from the prompts, one fused engine call per test batch -> (result, probabilities, metric)."""
    from ..evaluation import clip_load
    from ..evaluation.dataloader import construct_dataloader
    from ..evaluation.feature import extract_text_features, zeroshot_scores
    if not torch.cuda.is_available():
        raise SystemExit(f"{feature_file_path(cfg)} not found and no GPU to extract features with: the image tower runs only in "
                         "the HIP engine")
    model, _ = clip_load.plain_load(cfg.MODEL.NAME, jit=False)
    wf = cfg.MODEL.get("WEIGHT_FORMAT", None)
    if wf is not None:
        model.visual.weight_format = str(wf)
    text_features = extract_text_features(cfg, tokenizer, model=model, return_numpy=False, class_names=class_names)
    loader = construct_dataloader(cfg, test_split_only=True)
    probs, _, labels = zeroshot_scores(cfg, model, loader, text_features)
    metric = get_metric(cfg.TEST.METRIC)
    return metric(np.squeeze(labels), probs), torch.from_numpy(probs), metric.__name__


def write_predictions(cfg, exp_name, test_predictions):
    stats = cfg.MODEL.get("STATS", None) or {}
    results = {
        "model_name": f"CLIP-{cfg.MODEL.NAME}", "dataset_name": cfg.DATASET.DATASET, "num_trainable_params": 0,
        "num_params": stats.get("n_params", None), "num_visual_params": stats.get("n_visual_params", None),
        "num_backbone_params": stats.get("n_backbone_params", None), "n_shot": 0, "rnd_seeds": [0],
        "predictions": [test_predictions.cpu().data.numpy().tolist()],
    }
    folder = os.path.join(cfg.OUTPUT_DIR, "predictions", exp_name)
    os.makedirs(folder, exist_ok=True)
    path = os.path.join(folder, f"{cfg.DATASET.DATASET}.json")
    with open(path, "w") as f:
        f.write(json_prec_dump(results))
    return path


def main(argv=None, tokenizer=None, class_names=None):
    """``tokenizer(texts, context_length=...)`` and ``class_names`` (strings, or already tokenised (T, context) tensors per class)
    are the caller's: the BPE vocabulary and the class tables belong to the reference's dataset layer.  Returns
    (result, probabilities, metric name)."""
    parser = argparse.ArgumentParser(description="Zero-shot evaluation script.")
    add_zero_shot_args(parser)
    args = parser.parse_args(argv)
    if args.ds:
        args.cfg = args.ds
        update_config(config, args)
    args.cfg = args.model
    update_config(config, args)
    config.defrost()
    config.NAME = ""
    config.freeze()
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    if args.text_feature_only:
        raise SystemExit("--text_feature_only extracts the knowledge-augmented text dictionaries of the reference (Wiktionary / "
                         "GPT-3 sources); the knowledge sources are not part of this build")
    exp_name = experiment_name(config)
    feature_file = feature_file_path(config)
    logging.info(f"feature_file: {feature_file}")
    if os.path.exists(feature_file):
        logging.info("Loading features from existing files.")
        with open(feature_file, "rb") as fread:
            image_features = np.load(fread)
            text_features = np.load(fread)
            image_labels = np.load(fread)
        logging.info(f"Test size is {image_features.shape[0]}.")
        result, test_predictions, metric = clip_zeroshot_evaluator(image_features, text_features, image_labels, config)
    else:
        result, test_predictions, metric = score_on_engine(config, tokenizer, class_names)
        logging.info(f"Test size is {test_predictions.shape[0]}.")
    logging.info(f"=> TEST: {metric} {100 * result:.3f}% ")
    if args.save_predictions:
        path = write_predictions(config, exp_name, test_predictions)
        logging.info(f"predictions written to {path}")
    return result, test_predictions, metric


if __name__ == "__main__":
    main()
