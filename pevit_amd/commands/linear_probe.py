"""python -m pevit_amd.commands.linear_probe --ds <dataset.yaml> --model <model.yaml> [--no-tuning True --lr .. --l2 ..]
[--emulate-zeroshot True] [KEY VALUE ...]   (reference: commands/linear_probe.py): the linear-probe baseline every PEFT number is
compared with -- a BatchNorm1d + Linear head on the frozen CLIP image tower (``TRAIN.FREEZE_IMAGE_BACKBONE True``, which the
reference's model yaml sets).

Same flags, same config layering (dataset yaml <- model yaml <- KEY VALUE opts), same output file
``<OUTPUT_DIR>/predictions/linear_probe_<n>/seed<S>_<dataset>.json`` with the reference's nine keys.  The work is
``evaluation.full_model_finetune``: with this project's tensor archives every image goes through the tower once per checkpoint
and every step after that trains the head on cached feature rows (``TRAIN.CACHE_FEATURES``)."""
from __future__ import annotations

import argparse
import logging
import os
import random

import numpy as np
import torch

from ..config import config, update_config
from ..evaluation.dataloader import construct_dataloader
from ._finetune import json_prec_dump


def add_linear_probing_args(parser):
    parser.add_argument("--ds", required=False, help="Evaluation dataset configure file name.", type=str)
    parser.add_argument("--model", required=True, help="Evaluation model configure file name", type=str)
    parser.add_argument("--submit-predictions", help="submit predictions and model info to leaderboard.", default=False,
                        action="store_true")
    parser.add_argument("--submit-by", help="Person who submits the results.", type=str)
    parser.add_argument("--no-tuning", help="No hyperparameter-tuning.", default=False, type=lambda x: x.lower() == "true")
    parser.add_argument("--emulate-zeroshot", help="Emulate zero shot learning.", default=False, type=str)
    parser.add_argument("--l2", help="(Inverse) L2 regularization strength; used when --no-tuning is True.", default=0.316, type=float)
    parser.add_argument("--lr", help="Learning rate; used when --no-tuning is True.", default=0.001, type=float)
    parser.add_argument("--run", help="Run id", default=1, type=int)
    parser.add_argument("--fix_seed", help="Fix the random seed. [-1] not fixing the seeds", default=0, type=int)
    parser.add_argument("--save-predictions", help="save predictions logits for analysis.", default=True, action="store_true")
    parser.add_argument("opts", help="Modify config options using the command-line", default=None, nargs=argparse.REMAINDER)


def experiment_name(cfg):
    """linear_probe.py:72-73 of the reference: 0 shots (--emulate-zeroshot) is a number, only a negative count reads 'full'"""
    n = cfg.DATASET.NUM_SAMPLES_PER_CLASS
    return "linear_probe_" + (str(n) if n >= 0 else "full")


def prepare(argv=None):
    """Parse the flags and layer the config the way the reference's main() does, up to the point where it builds the loaders:
    (args, experiment name)."""
    parser = argparse.ArgumentParser(description="Test a classification model, with linear probing.")
    add_linear_probing_args(parser)
    args = parser.parse_args(argv)
    if args.ds:
        args.cfg = args.ds
        update_config(config, args)
    args.cfg = args.model
    update_config(config, args)
    config.defrost()
    config.NAME = ""
    config.freeze()
    if args.submit_predictions:
        raise SystemExit("--submit-predictions talks to the reference's leaderboard service; not available here")
    if args.fix_seed != -1:
        random.seed(args.fix_seed); np.random.seed(args.fix_seed)
        torch.manual_seed(args.fix_seed); torch.cuda.manual_seed_all(args.fix_seed)
    if args.emulate_zeroshot:
        args.no_tuning = True
        config.defrost()
        config.TRAIN.END_EPOCH = 1
        config.TRAIN.EXTRA_FINAL_TRAIN_EPOCH = 0
        config.DATASET.NUM_SAMPLES_PER_CLASS = 0
        config.TRAIN.EMULATE_ZERO_SHOT = True
        config.freeze()
    exp_name = experiment_name(config)                 # (named before the 1 -> 2 rule, as in the reference)
    if config.DATASET.NUM_SAMPLES_PER_CLASS == 1:
        config.defrost()
        config.DATASET.NUM_SAMPLES_PER_CLASS = 2
        config.DATASET.MERGE_TRAIN_VAL_FINAL_RUN = False
        config.freeze()
    if config.DATASET.DATASET == "patch-camelyon" and config.DATASET.NUM_SAMPLES_PER_CLASS == -1:
        # the large set: search on a 10000-shot subset (the final run on the full set needs the reference's dataset layer)
        config.defrost()
        config.DATASET.NUM_SAMPLES_PER_CLASS = 10000
        config.freeze()
    return args, exp_name


def write_results(cfg, exp_name, model_info):
    results = {
        "model_name": cfg.MODEL.NAME, "dataset_name": cfg.DATASET.DATASET,
        "num_trainable_params": model_info.get("n_trainable_params", None), "num_params": model_info.get("n_params", None),
        "num_visual_params": model_info.get("n_visual_params", None),
        "num_backbone_params": model_info.get("n_backbone_params", None),
        "n_shot": cfg.DATASET.NUM_SAMPLES_PER_CLASS, "rnd_seeds": [cfg.DATASET.RANDOM_SEED_SAMPLING],
        "predictions": [np.asarray(model_info["best_logits"]).tolist()],
    }
    folder = os.path.join(cfg.OUTPUT_DIR, "predictions", exp_name)
    os.makedirs(folder, exist_ok=True)
    path = os.path.join(folder, f"seed{cfg.DATASET.RANDOM_SEED_SAMPLING}_{cfg.DATASET.DATASET}.json")
    with open(path, "w") as f:
        f.write(json_prec_dump(results))
    return path


def main(argv=None, entry=None):
    """``entry``: what runs the probe (default ``evaluation.full_model_finetune.full_model_finetune``)."""
    args, exp_name = prepare(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    logging.info(f"{config.DATASET.DATASET} is a dataset.")
    train_dl, val_dl, test_dl = construct_dataloader(config)
    if entry is None:
        from ..evaluation.full_model_finetune import full_model_finetune as entry
    best_acc, model_info = entry(train_dl, val_dl, test_dl, args.no_tuning, args.lr, args.l2, config)
    if args.save_predictions:
        path = write_results(config, exp_name, model_info)
        logging.info(f"results written to {path}")
    return best_acc, model_info


if __name__ == "__main__":
    main()
