"""Linear-probe rates on the engine (ViT-B/32, synthetic weights, 100 classes, 500 train + 10,000 test rows, resident f32 images).

  run    seconds per 50-epoch run (every epoch: the train rows in batches of 64, then a validation on the test rows) for two legs:
           uncached  every step runs the tower: HipEngine.train_step on the images, validation = 79 HipEngine.predict calls of 128
                     (only calls that exist on a tree without the probe kernels: --baseline-only runs this leg alone there)
           cached    the feature extraction (encode_image in chunks of 128 over all 10,500 images, INCLUDED in the time), then
                     probe_step on the cached rows and ONE probe_predict per validation
  step   microseconds per step by HIP events over --step-iters back-to-back steps: probe_step against the chain
         head_forward_backward(need_dfeat=False) + sgd_step on the same (pre-gathered) feature rows, B = 64 and 128, C = 100, D = 512
  val    probe_predict over the 10,000 cached rows against 79 predict calls of 128 images

Every leg runs one warm-up (a 2-epoch run), then --rounds timed rounds in alternation; wall clock is taken between synchronises.
--one-pass ROUTE (probe | chain): nothing but --step-iters head steps of that route at B = 128 on random feature rows (the process to
put under rocprofv3 --kernel-trace --stats).
Prints one JSON object.  usage: python scripts/probe_rate.py [--epochs 50] [--rounds 3] [--baseline-only] [--one-pass ROUTE] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C, N_TRAIN, N_TEST, BS, VBS = 100, 500, 10000, 64, 128


def sync():
    torch.cuda.synchronize()


def fresh(eng):
    eng.reset_run()
    g = torch.Generator().manual_seed(3)
    v = eng.param_views()
    with torch.no_grad():
        v["layers.0.weight"].copy_((torch.randn(v["layers.0.weight"].shape, generator=g) * 0.02).cuda())


def run_uncached(eng, tr_x, tr_y, te_x, epochs):
    fresh(eng)
    g = torch.Generator().manual_seed(0)
    for _ in range(epochs):
        order = torch.randperm(N_TRAIN, generator=g).cuda()
        for lo in range(0, N_TRAIN, BS):
            sel = order[lo:lo + BS]
            eng.train_step(tr_x[sel], tr_y[sel], lr=0.01, momentum=0.9, weight_decay=1e-4)
        for lo in range(0, N_TEST, VBS):
            eng.predict(te_x[lo:lo + VBS])


def run_cached(eng, tr_x, tr_y, te_x, epochs):
    fresh(eng)
    D = eng.arch.embed_dim
    tr_f = torch.empty((N_TRAIN, D), device="cuda"); te_f = torch.empty((N_TEST, D), device="cuda")
    for x, f in ((tr_x, tr_f), (te_x, te_f)):
        for lo in range(0, x.shape[0], VBS):
            f[lo:lo + VBS] = eng.encode_image(x[lo:lo + VBS])
    g = torch.Generator().manual_seed(0)
    for _ in range(epochs):
        order = torch.randperm(N_TRAIN, generator=g).cuda()
        for lo in range(0, N_TRAIN, BS):
            eng.probe_step(tr_f, order[lo:lo + BS].contiguous(), tr_y, lr=0.01, momentum=0.9, weight_decay=1e-4)
        eng.probe_predict(te_f)
    return tr_f, te_f


def timed(fn):
    sync(); t = time.perf_counter(); fn(); sync()
    return time.perf_counter() - t


def events_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    sync(); a.record()
    for _ in range(iters):
        fn()
    b.record(); sync()
    return a.elapsed_time(b) * 1e3 / iters


def spread(xs):
    return {"min": min(xs), "max": max(xs), "rounds": xs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-iters", type=int, default=200)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--one-pass", choices=["probe", "chain"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pevit_amd.engine import HipEngine
    from pevit_amd.synth import ARCHS, synth_state_dict
    arch = ARCHS["ViT-B/32"]
    eng = HipEngine(arch, "none", C, VBS)
    eng.load_state_dict(synth_state_dict(arch))
    g = torch.Generator().manual_seed(1)
    if args.one_pass:
        f = torch.randn((N_TRAIN, arch.embed_dim), generator=g).cuda(); y = (torch.arange(N_TRAIN) % C).cuda()
        idx = torch.randperm(N_TRAIN, generator=g)[:128].cuda()
        fb, yb = f[idx].contiguous(), y[idx].contiguous()
        fresh(eng)
        for _ in range(args.step_iters):
            if args.one_pass == "probe":
                eng.probe_step(f, idx, y, lr=0.01, momentum=0.9, weight_decay=1e-4)
            else:
                eng.head_forward_backward(fb, yb, need_dfeat=False)
                eng.sgd_step(0.01, 0.9, 1e-4)
        sync()
        print(json.dumps({"one_pass": args.one_pass, "steps": args.step_iters}))
        return
    tr_x = torch.randn((N_TRAIN, 3, 224, 224), generator=g).cuda(); tr_y = (torch.arange(N_TRAIN) % C).cuda()
    te_x = torch.randn((N_TEST, 3, 224, 224), generator=g).cuda()
    out = {"epochs": args.epochs, "rounds": args.rounds, "baseline_only": args.baseline_only}
    legs = {"uncached": run_uncached} if args.baseline_only else {"uncached": run_uncached, "cached": run_cached}
    for fn in legs.values():
        fn(eng, tr_x, tr_y, te_x, 2)                                              # warm-up
    secs = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            secs[k].append(timed(lambda: fn(eng, tr_x, tr_y, te_x, args.epochs)))
    out["run_seconds"] = {k: spread(v) for k, v in secs.items()}
    if not args.baseline_only:
        tr_f, te_f = run_cached(eng, tr_x, tr_y, te_x, 1)
        out["step_us"] = {}
        for B in (64, 128):
            idx = torch.randperm(N_TRAIN, generator=g)[:B].cuda()
            fb, yb = tr_f[idx].contiguous(), tr_y[idx].contiguous()

            def chain():
                eng.head_forward_backward(fb, yb, need_dfeat=False)
                eng.sgd_step(0.01, 0.9, 1e-4)

            def probe():
                eng.probe_step(tr_f, idx, tr_y, lr=0.01, momentum=0.9, weight_decay=1e-4)
            fresh(eng); chain(); probe()
            us = {"chain": [], "probe_step": []}
            for _ in range(args.rounds):
                us["chain"].append(events_us(chain, args.step_iters))
                us["probe_step"].append(events_us(probe, args.step_iters))
            out["step_us"][f"B{B}"] = {k: spread(v) for k, v in us.items()}

        def val_calls():
            for lo in range(0, N_TEST, VBS):
                eng.predict(te_x[lo:lo + VBS])
        v = {"predict_79_calls": [], "probe_predict": []}
        val_calls(); eng.probe_predict(te_f)
        for _ in range(args.rounds):
            v["predict_79_calls"].append(timed(val_calls) * 1e3)
            v["probe_predict"].append(timed(lambda: eng.probe_predict(te_f)) * 1e3)
        out["validation_ms"] = {k: spread(x) for k, x in v.items()}
    text = json.dumps(out)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
