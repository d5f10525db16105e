"""train_one images/s by optimizer route (ViT-B/32 + KAdaptation and + LoRA, 100 classes, batch 64 and 128):

  sgd               torch.optim.SGD, one set of hyper-parameters: the fused step with sgd_kernel (ClassifierBase.can_fuse)
  adamw_fused       TRAIN.OPTIMIZER adamW: fused forward/backward + optim_kernel (ClassifierBase.fused_optimizer_plan)
  adamw_torch       the same optimizer with TRAIN.FUSED_OPTIMIZER False: engine forward, BatchNorm + Linear + loss in torch, engine
                    backward, torch.optim.AdamW.step() -- the only route for it before the fused optimizer step existed
  sgd_two_wd_fused  TRAIN.WITHOUT_WD_LIST ['bias'] (two weight decays): fused forward/backward + optim_kernel
  sgd_two_wd_torch  the same with TRAIN.FUSED_OPTIMIZER False

Each route runs one warm-up epoch, then REPS timed epochs in alternation (route order rotated every repetition), each epoch STEPS
full batches of a resident f32 TensorLoader; the engine's optimizer state is reset before every epoch (it belongs to one optimizer
kind at a time).  ``--profile``: additionally brackets single launches of the fused optimizer kernel with device events (gradients
as the last step left them) and reports the median microseconds per launch.  Prints one JSON object.
usage: python scripts/optimizer_rate.py [--steps 20] [--reps 5] [--profile] [--out FILE]"""
import argparse
import dataclasses
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUTES = ("sgd", "adamw_fused", "adamw_torch", "sgd_two_wd_fused", "sgd_two_wd_torch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--methods", default="kadaptation,lora")
    ap.add_argument("--batches", default="64,128")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pevit_amd.config import vitb32_clip_config
    from pevit_amd.evaluation import _harness
    from pevit_amd.evaluation.dataloader import TensorLoader, _Tensors
    from pevit_amd.optim import build_optimizer
    from pevit_amd.synth import ARCHS, synth_state_dict
    dev, C = torch.device("cuda", 0), 100
    arch = dataclasses.replace(ARCHS["ViT-B/32"], text_layers=1)
    crit = torch.nn.CrossEntropyLoss()
    out = {"how": f"train_one, {args.steps} full batches per epoch of a resident f32 TensorLoader (shuffle on), ViT-B/32, {C} classes; "
                  f"one warm-up epoch per route, then {args.reps} timed epochs per route in rotated alternation"}
    with tempfile.TemporaryDirectory() as tmp:
        ckpt = os.path.join(tmp, "vitb32_synth.pt")
        torch.save(synth_state_dict(arch, seed=2, text_tower=True), ckpt)
        for method in args.methods.split(","):
            mod = importlib.import_module("pevit_amd.evaluation." + {"kadaptation": "kadaptation_clip", "lora": "lora_clip"}[method])
            cfg = vitb32_clip_config()
            cfg.MODEL.NAME = ckpt
            cfg.DATASET.NUM_CLASSES = C
            cfg.TRAIN.LR, cfg.TRAIN.WD = 1e-3, 1e-4
            cfg.GPUS = (0,)
            model = mod.Classifier(cfg, 0).cuda(dev)
            opts = {}
            for name, over in (("sgd", {}), ("adamw", {"OPTIMIZER": "adamW"}), ("sgd_two_wd", {"WITHOUT_WD_LIST": ["bias"]})):
                c = cfg.clone()
                for k, v in over.items():
                    setattr(c.TRAIN, k, v)
                opts[name] = build_optimizer(c, model)
            assert model.can_fuse(crit, opts["sgd"])
            for name in ("adamw", "sgd_two_wd"):
                assert not model.can_fuse(crit, opts[name]) and model.fused_optimizer_plan(crit, opts[name]) is not None

            def epoch(route, loader, ep):
                model._fused_optimizer = not route.endswith("_torch")        # what TRAIN.FUSED_OPTIMIZER sets on the Classifier
                opt = opts[route.rsplit("_", 1)[0] if route != "sgd" else "sgd"]
                model.engine().reset_optimizer()
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                mod.train_one(loader, model, crit, opt, ep, cfg)
                torch.cuda.synchronize(dev)
                return time.perf_counter() - t0

            g = torch.Generator().manual_seed(0)
            res_m = {}
            for bs in (int(b) for b in args.batches.split(",")):
                n = args.steps * bs
                x = torch.randn((n, 3, 224, 224), generator=g).to(dev)
                y = torch.randint(0, C, (n,), generator=g).to(dev)
                loader = TensorLoader(_Tensors(x, y), batch_size=bs, shuffle=True)
                rates = {r: [] for r in ROUTES}
                for r in ROUTES:
                    epoch(r, loader, 0)                                       # warm-up epoch
                for rep in range(args.reps):
                    k = rep % len(ROUTES)
                    for r in ROUTES[k:] + ROUTES[:k]:
                        rates[r].append(n / epoch(r, loader, 1))
                res = {r: {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": [round(a, 1) for a in v]}
                       for r, v in rates.items()}
                for name in ("adamw", "sgd_two_wd"):
                    res[f"{name}_fused_over_torch"] = res[name + "_fused"]["median"] / res[name + "_torch"]["median"]
                res["adamw_fused_over_sgd"] = res["adamw_fused"]["median"] / res["sgd"]["median"]
                res_m[f"bs{bs}"] = res
                del x, y, loader
            if args.profile:
                eng = model.engine()
                prof = {"n_params": eng.n_params}
                model._fused_optimizer = True
                for name in ("adamw", "sgd_two_wd"):
                    plan = model.fused_optimizer_plan(crit, opts[name])
                    eng.reset_optimizer()
                    for _ in range(5):
                        eng.optimizer_step(plan)
                    pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(100)]
                    for a, b in pairs:
                        a.record(); eng.optimizer_step(plan); b.record()
                    torch.cuda.synchronize(dev)
                    us = sorted(a.elapsed_time(b) * 1e3 for a, b in pairs)
                    prof[name] = {"optim_kernel_us_median": us[len(us) // 2], "min": us[0], "max": us[-1]}
                eng.reset_optimizer()
                pairs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(100)]
                for a, b in pairs:
                    a.record(); eng.sgd_step(1e-3); b.record()
                torch.cuda.synchronize(dev)
                us = sorted(a.elapsed_time(b) * 1e3 for a, b in pairs)
                prof["sgd"] = {"sgd_kernel_us_median": us[len(us) // 2], "min": us[0], "max": us[-1]}
                res_m["profile"] = prof
            out[method] = res_m
            del model, opts
            _harness._BACKBONES.clear()
    s = json.dumps(out, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
