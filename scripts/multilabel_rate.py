"""train_one images/s of a multi-label fine-tune (ViT-B/32 + KAdaptation, 20 classes, seeded multi-hot targets) by route:

  fused_bce     BCEWithLogitsLoss(): the fused engine step with bce_loss_kernel (pevit_train_forward_backward_bce)
  autograd_bce  BCEWithLogitsLoss(pos_weight=ones(C)): the same loss value, not fused -- engine forward, BatchNorm + Linear + loss
                in torch, engine backward, torch.optim.SGD
  ce            CrossEntropyLoss() on class indices at the same batch and class count: the single-label fused step

Each route runs one warm-up epoch, then REPS timed epochs in alternation (route order rotated every repetition), each epoch STEPS
full batches of a resident f32 TensorLoader.  Prints one JSON object: per batch size and route the median, min and max images/s.
usage: python scripts/multilabel_rate.py [--steps 20] [--reps 5] [--out FILE]"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pevit_amd.config import vitb32_clip_config
    from pevit_amd.evaluation import _harness, kadaptation_clip as mod
    from pevit_amd.evaluation.dataloader import TensorLoader, _Tensors
    from pevit_amd.optim import build_optimizer
    from pevit_amd.synth import ARCHS, synth_state_dict
    dev, C = torch.device("cuda", 0), 20
    arch = dataclasses.replace(ARCHS["ViT-B/32"], text_layers=1)
    out = {"how": f"train_one, {args.steps} full batches per epoch of a resident f32 TensorLoader (shuffle on), ViT-B/32 + KAdaptation, "
                  f"{C} classes; one warm-up epoch per route, then {args.reps} timed epochs per route in rotated alternation"}
    with tempfile.TemporaryDirectory() as tmp:
        ckpt = os.path.join(tmp, "vitb32_synth.pt")
        torch.save(synth_state_dict(arch, seed=2, text_tower=True), ckpt)
        cfg = vitb32_clip_config()
        cfg.MODEL.NAME = ckpt
        cfg.DATASET.NUM_CLASSES = C
        cfg.TRAIN.LR, cfg.TRAIN.WD = 0.01, 1e-6
        cfg.GPUS = (0,)
        model = mod.Classifier(cfg, 0).cuda(dev)
        opt = build_optimizer(cfg, model)
        crits = {"fused_bce": torch.nn.BCEWithLogitsLoss(), "autograd_bce": torch.nn.BCEWithLogitsLoss(pos_weight=torch.ones(C, device=dev)),
                 "ce": torch.nn.CrossEntropyLoss()}
        assert model.can_fuse(crits["fused_bce"], opt) and not model.can_fuse(crits["autograd_bce"], opt)
        assert model.can_fuse(crits["ce"], opt)
        g = torch.Generator().manual_seed(0)
        for bs in (64, 128):
            n = args.steps * bs
            x = torch.randn((n, 3, 224, 224), generator=g).to(dev)
            y = (torch.rand((n, C), generator=g) < 0.1).float()
            y[torch.arange(n), torch.randint(0, C, (n,), generator=g)] = 1.0
            cls = torch.randint(0, C, (n,), generator=g)
            loaders = {"fused_bce": TensorLoader(_Tensors(x, y.to(dev)), batch_size=bs, shuffle=True),
                       "autograd_bce": TensorLoader(_Tensors(x, y.to(dev)), batch_size=bs, shuffle=True),
                       "ce": TensorLoader(_Tensors(x, cls.to(dev)), batch_size=bs, shuffle=True)}
            routes = list(crits)
            rates = {r: [] for r in routes}
            for r in routes:
                mod.train_one(loaders[r], model, crits[r], opt, 0, cfg)              # warm-up epoch
            for rep in range(args.reps):
                for r in routes[rep % 3:] + routes[:rep % 3]:
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    mod.train_one(loaders[r], model, crits[r], opt, 1, cfg)
                    torch.cuda.synchronize(dev)
                    rates[r].append(n / (time.perf_counter() - t0))
            res = {r: {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": [round(a, 1) for a in v]}
                   for r, v in rates.items()}
            res["fused_bce_over_ce"] = res["fused_bce"]["median"] / res["ce"]["median"]
            res["fused_bce_over_autograd_bce"] = res["fused_bce"]["median"] / res["autograd_bce"]["median"]
            out[f"bs{bs}"] = res
            del x, loaders
        del model, opt
        _harness._BACKBONES.clear()
    s = json.dumps(out, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
