"""Gradient-norm clipping: what the two launches cost, and what they cost the step.

  pair     microseconds per clip launch pair (grad_sumsq_kernel + grad_scale_kernel, ``pevit_op_clip_grad_norm``) on flat f32
           buffers of the sizes the methods train -- 1.0e5 (KAdaptation + head) to a few million (bottleneck Adapter on ViT-L/14)
           -- against their byte floor: one read plus one read-modify-write of 4n bytes at 6.3 TB/s.  Device events around runs of
           PAIRS_PER_WINDOW pairs, the median over the windows; with a mask (one more byte read per element and launch) and without.
  step     images/s of the headline step (ViT-B/32 + KAdaptation, 100 classes, batch 128, ``HipEngine.train_step``) with
           ``HipEngine.max_grad_norm`` set against None, in alternation; the bound never binds (1e9), which costs what a binding one costs: the
           product is always taken.
  norm     the distance of the norm from f64 in units of 2^-24, the engine's and torch's f32 ``clip_grad_norm_``, on the buffers of
           tests/test_gpu_clip.py.

Prints one JSON object.   usage: python scripts/clip_rate.py [--steps 30] [--reps 5] [--out FILE]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.3e12
PAIRS_PER_WINDOW, WINDOWS = 50, 21
SIZES = (100_000, 1_000_000, 3_000_000, 8_000_000)


def pair_times(lib, _lib):
    out = {}
    for n in SIZES:
        for masked in (False, True):
            g = torch.randn(n, device="cuda")
            mask = (torch.rand(n, device="cuda") < 0.9).to(torch.uint8) if masked else None
            scratch = torch.zeros(lib.pevit_clip_scratch_floats(n), device="cuda")

            def pair():
                rc = lib.pevit_op_clip_grad_norm(_lib.stream_ptr(), _lib.ptr(g), _lib.ptr(mask), n, 1e9, 1.0, _lib.ptr(scratch))
                assert rc == 0, lib.pevit_last_error()
            for _ in range(20):
                pair()
            us = []
            for _ in range(WINDOWS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(PAIRS_PER_WINDOW):
                    pair()
                b.record()
                torch.cuda.synchronize()
                us.append(a.elapsed_time(b) * 1e3 / PAIRS_PER_WINDOW)
            floor = (3 * 4 * n + (2 * n if masked else 0)) / HBM_BYTES_PER_S * 1e6
            out[f"n{n}{'_masked' if masked else ''}"] = {"us_per_pair_median": statistics.median(us), "min": min(us), "max": max(us),
                                                        "byte_floor_us": floor, "workgroups": int(scratch.numel()) - 4}
    return out


def step_rates(steps, reps):
    import dataclasses
    from pevit_amd.engine import HipEngine, adapter_param_spec
    from pevit_amd.synth import ARCHS, randomize_adapters, synth_batch, synth_state_dict
    arch, method, B, C = dataclasses.replace(ARCHS["ViT-B/32"], text_layers=1), "kadaptation", 128, 100
    sd = {k: v for k, v in synth_state_dict(arch, seed=2, text_tower=False).items() if k.startswith("visual.")}
    ad = [(n, torch.zeros(s)) for n, s, _ in adapter_param_spec(method, arch.width, arch.layers)]
    randomize_adapters(ad, seed=3); sd.update(dict(ad))
    eng = HipEngine(arch, method, C, B)
    eng.load_state_dict(sd)
    images, labels = synth_batch(B, arch.resolution, C)
    images, labels = images.cuda(), labels.cuda()

    def window(clip):
        eng.max_grad_norm = clip
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            eng.train_step(images, labels, lr=1e-3, momentum=0.9, weight_decay=1e-4)
        b.record()
        torch.cuda.synchronize()
        return steps * B / (a.elapsed_time(b) * 1e-3)
    off, on = None, 1e9
    for clip in (off, on, off, on):
        window(clip)                                            # warm-up
    rates = {"off": [], "on": []}
    for rep in range(reps):
        for name, clip in (("off", off), ("on", on)) if rep % 2 == 0 else (("on", on), ("off", off)):
            rates[name].append(window(clip))
    res = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": [round(x, 1) for x in v]} for k, v in rates.items()}
    res["on_over_off"] = res["on"]["median"] / res["off"]["median"]
    res["n_params"] = eng.n_params
    res["how"] = f"{steps} steps per window, {reps} windows each in alternation, batch {B}"
    return res


def norm_distances(lib, _lib):
    chunk, u = 8192, 2.0 ** -24
    out = {}
    for n in (1, 3, 63, 64, 65, 1023, chunk - 1, chunk, chunk + 1, 3 * chunk + 5, 2 ** 20 + 3):
        g = torch.Generator().manual_seed(n)
        v = torch.randn(n, generator=g) * 10.0 ** (torch.rand(n, generator=g) * 9.0 - 6.0)
        ref = float(v.double().square().sum().sqrt())
        buf, scratch = v.cuda(), torch.zeros(lib.pevit_clip_scratch_floats(n), device="cuda")
        assert lib.pevit_op_clip_grad_norm(_lib.stream_ptr(), _lib.ptr(buf), None, n, 1e30, 1.0, _lib.ptr(scratch)) == 0
        p = torch.nn.Parameter(torch.zeros(n, device="cuda")); p.grad = v.cuda()
        t = float(torch.nn.utils.clip_grad_norm_([p], 1e30))
        out[f"n{n}"] = {"engine_u": abs(float(scratch[0]) - ref) / ref / u, "torch_f32_u": abs(t - ref) / ref / u,
                        "gate_u": math.ceil(math.log2(n)) + 3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pevit_amd import _lib
    lib = _lib.load()
    out = {"pair": pair_times(lib, _lib), "norm": norm_distances(lib, _lib), "step": step_rates(args.steps, args.reps)}
    s = json.dumps(out, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
