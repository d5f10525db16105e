"""Zero-shot images/s of the two routes from images to class probabilities (ViT-B/32, method none, synthetic weights, resident f32
images):

  torch   what a user could do before the zero-shot path: model.encode_image (pevit_visual_forward(save = 0), the training kernel
          forms) + F.normalize + matmul + softmax as torch launches
  engine  HipEngine.zeroshot: one pevit_zeroshot call (the tower's inference forms + the cosine head and its softmax in one launch)

Configurations: batch 64 (the loader's) and 128, C = 100 and 1000 classes.  Each route runs one warm-up pass, then REPS timed passes
in alternation (the order swaps every repetition), a pass being STEPS batches.  Wall clock is taken with a synchronise on both
sides; next to it the median over the batches of a HIP-event pair around each batch.  The probabilities of the two routes are
compared once per configuration (the tower kernels differ only in what they store; the f32 tail is computed by different code).

--one-pass ROUTE: nothing but a warm-up and one pass of ROUTE at batch 128, C = 1000 (the process to put under
rocprofv3 --kernel-trace --stats; zeroshot_head_kernel's row is the new kernel's time).
Prints one JSON object.  usage: python scripts/zeroshot_rate.py [--steps 20] [--reps 3] [--out FILE]"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import tempfile
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(ckpt, max_batch):
    from pevit_amd.evaluation import clip_load
    model, _ = clip_load.plain_load(ckpt, device="cuda:0", jit=False)
    model.visual._max_batch = max_batch
    model.visual.engine()
    return model


def text_features(D, classes):
    g = torch.Generator().manual_seed(7)
    return F.normalize(torch.randn((D, classes), generator=g), dim=0).cuda()           # (D, C): unit columns, the reference's layout


def routes_for(model, text_dc):
    eng = model.visual.engine()
    text_cd = text_dc.t().contiguous()                                                 # class-major, once per evaluation
    return {"torch": lambda b: (100. * F.normalize(model.encode_image(b)) @ text_dc).softmax(dim=-1),
            "engine": lambda b: eng.zeroshot(b, text_cd)}


def run_pass(fn, batches, events=None):
    for i, x in enumerate(batches):
        if events is not None:
            events[i][0].record()
        fn(x)
        if events is not None:
            events[i][1].record()


def measure(model, bs, classes, steps, reps):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    x = torch.randn((steps * bs, 3, 224, 224), generator=g).to(dev)
    batches = [x[i * bs:(i + 1) * bs] for i in range(steps)]
    routes = routes_for(model, text_features(model.visual.output_dim, classes))
    with torch.no_grad():
        a, b = routes["torch"](batches[0]), routes["engine"](batches[0])
        torch.cuda.synchronize(dev)
        agree = float((a - b).abs().max() / a.abs().max())
        for r in routes.values():
            run_pass(r, batches)                                  # warm-up pass
        wall = {r: [] for r in routes}
        ev_us = {r: [] for r in routes}
        order = list(routes)
        for rep in range(reps):
            for r in (order if rep % 2 == 0 else order[::-1]):
                events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in batches]
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                run_pass(routes[r], batches, events)
                torch.cuda.synchronize(dev)
                wall[r].append(steps * bs / (time.perf_counter() - t0))
                ev_us[r].append(statistics.median(s.elapsed_time(e) * 1e3 for s, e in events))
    res = {r: {"images_per_s_median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1),
               "rounds": [round(q, 1) for q in v], "event_us_per_batch_median": round(statistics.median(ev_us[r]), 1),
               "event_us_per_batch_rounds": [round(q, 1) for q in ev_us[r]]} for r, v in wall.items()}
    res["engine_over_torch"] = round(res["engine"]["images_per_s_median"] / res["torch"]["images_per_s_median"], 4)
    # accepted when the engine route's median is not below the slowest pass of the torch route on this visit
    res["engine_median_over_torch_min"] = round(res["engine"]["images_per_s_median"] / res["torch"]["min"], 4)
    res["probabilities_max_rel_difference"] = agree
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--one-pass", choices=["torch", "engine"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pevit_amd.synth import ARCHS, synth_state_dict
    arch = dataclasses.replace(ARCHS["ViT-B/32"], text_layers=1)
    out = {"how": f"ViT-B/32, method none, synthetic weights, resident f32 images; a pass = {args.steps} batches; one warm-up pass per "
                  f"route, then {args.reps} timed passes per route in alternation; wall clock between two synchronises"}
    with tempfile.TemporaryDirectory() as tmp:
        ckpt = os.path.join(tmp, "vitb32_synth.pt")
        torch.save(synth_state_dict(arch, seed=2, text_tower=True), ckpt)
        model = build(ckpt, 128)
        if args.one_pass:
            x = torch.randn((128, 3, 224, 224), generator=torch.Generator().manual_seed(0)).cuda()
            fn = routes_for(model, text_features(model.visual.output_dim, 1000))[args.one_pass]
            with torch.no_grad():
                for _ in range(1 + args.steps):
                    fn(x)
            torch.cuda.synchronize()
            print(json.dumps({"one_pass": args.one_pass, "forwards": 1 + args.steps, "batch": 128, "classes": 1000}))
            return
        for bs in (64, 128):
            for classes in (100, 1000):
                out[f"bs{bs}_c{classes}"] = measure(model, bs, classes, args.steps, args.reps)
    s = json.dumps(out, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
