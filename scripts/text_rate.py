"""Seconds per zero-shot head extraction through the two routes of extract_text_features (ViT-B/32 text tower at its real size:
width 512, 12 layers, 8 heads, 77 tokens, vocabulary 49,408, output 512; synthetic weights; 18 templates per class):

  torch    today's route: CLIP.encode_text in f32, one call per class (18 prompts), then normalise / mean / normalise per class
  engine   CLIP.encode_text_engine: all prompts stacked, TextEngine.encode in chunks of --max-prompts (256), then
           reduce_class_features over the stacked tensor.  The engine is built (weights packed) once, before the passes; that
           one-time cost is reported next to the passes as engine_build_s.

Sizes: 1,800 prompts (100 classes) and 18,000 prompts (1,000 classes).  Per size each route runs one warm-up pass, then --reps
timed passes in alternation (the order swaps every repetition); a pass ends in a device synchronise.  The head weights of the two
routes are compared once per size.
--one-pass ROUTE: nothing but a warm-up and one pass of ROUTE at 1,800 prompts (the process to put under rocprofv3 --kernel-trace --stats).
Prints one JSON object.  usage: python scripts/text_rate.py [--reps 3] [--max-prompts 256] [--out FILE]"""
import argparse
import dataclasses
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TEMPLATES = 18


def prompts(classes, arch, seed=0):
    g = torch.Generator().manual_seed(seed)
    S, N, V = classes * TEMPLATES, arch.context_length, arch.vocab_size
    tok = torch.randint(1, V - 2, (S, N), generator=g)
    eot = torch.randint(3, N, (S,), generator=g)
    for s in range(S):
        tok[s, eot[s]] = V - 1
        tok[s, eot[s] + 1:] = 0
    return tok.cuda()


def torch_route(model, tok):
    cols = []
    for c in range(tok.shape[0] // TEMPLATES):
        e = model.encode_text(tok[c * TEMPLATES:(c + 1) * TEMPLATES])
        e = e / e.norm(dim=-1, keepdim=True)
        m = e.mean(dim=0)
        cols.append(m / m.norm())
    return torch.stack(cols, dim=1)


def engine_route(model, tok, index, max_prompts):
    from pevit_amd.evaluation.feature import reduce_class_features
    return reduce_class_features(model.encode_text_engine(tok, max_prompts=max_prompts), index, tok.shape[0] // TEMPLATES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-prompts", type=int, default=256)
    ap.add_argument("--one-pass", choices=["torch", "engine"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from pevit_amd.evaluation.model import build_model
    from pevit_amd.synth import ARCHS, synth_state_dict
    arch = dataclasses.replace(ARCHS["ViT-B/32"], layers=1)          # the image tower is not run here
    model = build_model(synth_state_dict(arch, seed=2, text_tower=True)).cuda(0)
    for p in model.parameters():
        p.requires_grad = False
    out = {"how": f"ViT-B/32 text tower (512 / 12 layers / 77 tokens / vocabulary 49,408 / out 512), synthetic weights, {TEMPLATES} "
                  f"templates per class; one warm-up pass per route, then {args.reps} timed passes per route in alternation; "
                  f"a pass is wall clock between two synchronises; engine chunks of {args.max_prompts} prompts"}
    with torch.no_grad():
        t0 = time.perf_counter()
        model.encode_text_engine(prompts(1, arch), max_prompts=args.max_prompts)
        torch.cuda.synchronize()
        out["engine_build_s"] = round(time.perf_counter() - t0, 4)       # context, arena, weight packing and a first call
        for classes in ((100,) if args.one_pass else (100, 1000)):
            tok = prompts(classes, arch)
            index = torch.arange(classes).repeat_interleave(TEMPLATES).cuda()
            routes = {"torch": lambda: torch_route(model, tok), "engine": lambda: engine_route(model, tok, index, args.max_prompts)}
            if args.one_pass:
                for _ in range(2):
                    routes[args.one_pass]()
                    torch.cuda.synchronize()
                print(json.dumps({"one_pass": args.one_pass, "extractions": 2, "prompts": int(tok.shape[0])}))
                return
            a, b = routes["torch"](), routes["engine"]()                 # (also the warm-up pass of both)
            torch.cuda.synchronize()
            secs = {r: [] for r in routes}
            order = list(routes)
            for rep in range(args.reps):
                for r in (order if rep % 2 == 0 else order[::-1]):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    routes[r]()
                    torch.cuda.synchronize()
                    secs[r].append(time.perf_counter() - t0)
            S = int(tok.shape[0])
            res = {r: {"seconds": [round(v, 4) for v in secs[r]], "prompts_per_s": [round(S / v, 1) for v in secs[r]]} for r in routes}
            res["slowest_engine_over_fastest_torch"] = round(max(secs["engine"]) / min(secs["torch"]), 4)
            res["head_max_rel_difference"] = float((a - b).abs().max() / a.abs().max())
            out[f"prompts_{S}"] = res
    s = json.dumps(out, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
