"""python -m pevit_amd.commands.predict --ds <dataset.yaml> --model <model.yaml> --adapter FILE [--save-predictions] [KEY VALUE ...]

Score the test split with a saved adapter (``TRAIN.SAVE_ADAPTER`` of the fine-tune commands, ``adapter_io.save_adapter``) next to
the frozen CLIP tower, on an engine context that can only infer (``serving.InferenceEngine``).  Same config layering as the other
commands (dataset yaml <- model yaml <- KEY VALUE opts).  The CLIP checkpoint is ``TEST.MODEL_FILE`` when set, else ``MODEL.NAME``
(a released model name or a file); method, LoRA rank, the tower's shapes, the class count and the input normalisation come from
the adapter file.  Scores with ``TEST.METRIC``, logs the result and writes
``<OUTPUT_DIR>/predictions/predict_<method>/<dataset>.json`` with the nine keys of the other commands' result files.
"""
from __future__ import annotations

import argparse
import logging
import os

import torch

from .. import adapter_io
from ..config import config, update_config
from ..evaluation.metric import get_metric
from ..synth import VitArch
from ._finetune import json_prec_dump


def add_predict_args(parser):
    parser.add_argument("--ds", required=False, help="Evaluation dataset configure file name.", type=str)
    parser.add_argument("--model", required=True, help="Clip model configure file name", type=str)
    parser.add_argument("--adapter", required=True, help="Adapter checkpoint written by TRAIN.SAVE_ADAPTER / save_adapter.", type=str)
    parser.add_argument("--save-predictions", help="save predictions logits for analysis.", default=True, action="store_true")
    parser.add_argument("opts", help="Modify config options using the command-line", default=None, nargs=argparse.REMAINDER)


def clip_state_dict(cfg):
    """The CLIP checkpoint the way the other commands read it: a released name is resolved in the cache, a path is read as it is."""
    from ..evaluation import clip_load
    name = cfg.TEST.get("MODEL_FILE", "") or cfg.MODEL.NAME
    if name in clip_load._MODELS:
        path = clip_load._resolve(*clip_load._MODELS[name], os.path.expanduser("~/.cache/clip"))
    elif os.path.isfile(name):
        path = name
    else:
        raise RuntimeError(f"Model {name} not found; available models = {clip_load.available_models()}")
    return clip_load._read_state_dict(path)


def build_engine(cfg, ckpt, sd):
    """An ``InferenceEngine`` shaped by the adapter's meta, the tower of ``sd`` loaded, the adapter resident and selected."""
    from ..serving import InferenceEngine
    meta = ckpt["meta"]
    arch = VitArch("custom", **adapter_io.arch_numbers(meta["arch"]))
    wf = cfg.MODEL.get("WEIGHT_FORMAT", None) or meta["weight_format"]
    # one engine call per batch of the test loader, as the harness's validate scores it (a row's bits may depend on its batch)
    max_batch = max(int(cfg.TEST.BATCH_SIZE_PER_GPU), int(cfg.DATASET.get("LOADER_BATCH_SIZE", 64)))
    eng = InferenceEngine(arch, meta["method"], max_classes=meta["num_classes"], max_batch=max_batch,
                          lora_rank=int(meta["lora_rank"]), device=torch.device("cuda", cfg.GPUS[0]), weight_format=str(wf))
    eng.set_input_normalization(meta["input_mean"], meta["input_std"])
    eng.set_input_resize(True, bool(meta["center_crop"]))
    eng.load_backbone(sd)
    eng.add_adapter("adapter", ckpt)
    eng.use("adapter")
    return eng


def score(cfg, eng):
    """(score in percent, softmax probabilities (n, C) as numpy, metric name) of the test split, as the harness's validate."""
    from ..evaluation._harness import DeviceFeeder, _score
    from ..evaluation.dataloader import construct_dataloader
    loader = construct_dataloader(cfg, test_split_only=True)
    outputs, targets = [], []
    for images, target in DeviceFeeder(loader, cfg.GPUS[0]):
        if not target.is_cuda:
            target = target.cuda(cfg.GPUS[0], non_blocking=True)
        if target.shape[-1] == 1:
            target = target[:, 0]
        outputs.append(eng.predict(images))
        targets.append(target)
    metric = get_metric(cfg.TEST.METRIC)
    result, probs = _score(metric, outputs, targets)
    return result, probs, metric.__name__


def write_predictions(cfg, ckpt, probs):
    meta = ckpt["meta"]
    results = {
        "model_name": cfg.MODEL.NAME, "dataset_name": cfg.DATASET.DATASET,
        "num_trainable_params": int(adapter_io.flat_params(ckpt).numel()), "num_params": None, "num_visual_params": None,
        "num_backbone_params": None, "n_shot": cfg.DATASET.NUM_SAMPLES_PER_CLASS, "rnd_seeds": [cfg.DATASET.RANDOM_SEED_SAMPLING],
        "predictions": [probs.tolist()],
    }
    folder = os.path.join(cfg.OUTPUT_DIR, "predictions", f"predict_{meta['method']}")
    os.makedirs(folder, exist_ok=True)
    path = os.path.join(folder, f"{cfg.DATASET.DATASET}.json")
    with open(path, "w") as f:
        f.write(json_prec_dump(results))
    return path


def main(argv=None):
    """Returns (score in percent, probabilities (n, C), metric name)."""
    parser = argparse.ArgumentParser(description="Score a dataset's test split with a saved adapter.")
    add_predict_args(parser)
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
    if not torch.cuda.is_available():
        raise SystemExit("predict needs a GPU: the image tower runs only in the HIP engine")
    ckpt = adapter_io.read_adapter(args.adapter)
    if ckpt["meta"]["dataset"] and ckpt["meta"]["dataset"] != config.DATASET.DATASET:
        logging.warning(f"the adapter was trained on {ckpt['meta']['dataset']!r}, scoring {config.DATASET.DATASET!r}")
    eng = build_engine(config, ckpt, clip_state_dict(config))
    result, probs, metric = score(config, eng)
    logging.info(f"Test size is {probs.shape[0]}.")
    logging.info(f"=> TEST: {metric} {result:.3f}% ")
    if args.save_predictions:
        logging.info(f"predictions written to {write_predictions(config, ckpt, probs)}")
    return result, probs, metric


if __name__ == "__main__":
    main()
