"""Evaluation images/s of the two routes validate() can take (ViT-B/32, synthetic weights, resident f32 images):

  module   the route before the inference path: Classifier.forward in eval mode under no_grad -- pevit_visual_forward(save = 0), which
           launches and stores exactly what the training forward does, then BatchNorm1d and Linear as torch launches
  predict  ClassifierBase.fused_predict: one pevit_predict call (the tower's inference forms + the engine's forward-only head)

Configurations: KAdaptation at batch 64, 128 and TEST.BATCH_SIZE_PER_GPU's default (32); Adapter at batch 128.  Each route runs one
warm-up pass, then REPS timed passes in alternation (the order swaps every repetition), a pass being STEPS batches.  Wall clock is
taken with a synchronise on both sides; next to it the median over the batches of a HIP-event pair around each batch.  The logits
of the two routes are compared once per configuration (the tower bits are the same; the f32 head is computed by different code).

--profile: additionally one batch per route under the engine's own per-launch events (HipEngine.profile_gemms(all_kernels=True)):
per kernel kind / GEMM shape the launches, milliseconds and ALGORITHMIC bytes (profile.hip prof_close) of a whole forward.
--one-pass ROUTE: nothing but a warm-up and one pass of ROUTE at batch 128 (the process to put under rocprofv3 --kernel-trace --stats).
--serving [--serving-route both|train|serving]: instead of the above, the serving leg (profiles/serving.md): ``HipEngine.predict``
on a training context ("train") against ``serving.InferenceEngine.predict`` on an inference-only one ("serving") -- ViT-B/32, KAdaptation,
100 classes, batches 128 and 32, REPS rounds each in alternation -- the arena / workspace bytes of both contexts as the library
reports them for ViT-B/32, ViT-B/16 and ViT-L/14 at batches 32 and 128, and microseconds per ``use()``.  With one route only, that
route alone is built and timed (a process per round, to alternate two builds of the library).
--segments: instead of the above, the segmented leg (profiles/serving.md; ``segments_leg`` below): eight requests of 16 images for
eight resident adapters as a loop of ``use`` + ``predict`` against ONE ``predict_segments`` call, and the cost of a ``slots = 8``
context.  --segments-one-pass ROUTE: nothing but STEPS calls of that route (the process to put under rocprofv3).
--method kadaptation|lora|adapter|compacter: the method of the --serving and --segments legs (default kadaptation; the post-MLP
methods: profiles/serving_segments.md).
Prints one JSON object.  usage: python scripts/predict_rate.py [--steps 20] [--reps 3] [--profile] [--serving] [--out FILE]"""
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

EPI_NAMES = {0: "qkv", 1: "bias_resid (out_proj / c_proj)", 2: "c_fc bias_gelu (h + g)", 4: "f32", 9: "bias_resid_keep",
             14: "c_fc bias_gelu_only (g)"}


def build(method, ckpt, max_batch):
    import importlib
    from pevit_amd.config import vitb32_clip_config
    mod = importlib.import_module("pevit_amd.evaluation." + {"kadaptation": "kadaptation_clip", "adapter": "adapter_tuning_clip"}[method])
    cfg = vitb32_clip_config()
    cfg.MODEL.NAME = ckpt
    cfg.DATASET.NUM_CLASSES = 100
    cfg.TEST.BATCH_SIZE_PER_GPU = max_batch
    cfg.GPUS = (0,)
    model = mod.Classifier(cfg, 0).cuda(0)
    model.eval()
    with torch.no_grad():       # non-trivial running statistics and adapters, so that the compared logits mean something
        g = torch.Generator().manual_seed(1)
        model.engine()
        model.channel_bn.running_mean.copy_((torch.randn(512, generator=g) * 0.3).cuda())
        model.channel_bn.running_var.copy_((0.5 + torch.rand(512, generator=g)).cuda())
        for n, p in model.backbone.named_parameters():
            if p.requires_grad:
                p.copy_((torch.randn(p.shape, generator=g) * 0.02).cuda())
    return model


def run_pass(fn, batches, events=None):
    for i, x in enumerate(batches):
        if events is not None:
            events[i][0].record()
        fn(x)
        if events is not None:
            events[i][1].record()


def measure(model, bs, steps, reps):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    x = torch.randn((steps * bs, 3, 224, 224), generator=g).to(dev)
    batches = [x[i * bs:(i + 1) * bs] for i in range(steps)]
    routes = {"module": lambda b: model(b), "predict": model.fused_predict}
    assert model.can_fuse_eval(batches[0])
    with torch.no_grad():
        a, b = routes["module"](batches[0]), routes["predict"](batches[0])
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
    res["predict_over_module"] = round(res["predict"]["images_per_s_median"] / res["module"]["images_per_s_median"], 4)
    # "not slower": no predict round below the slowest round of the module route on this box
    res["predict_min_over_module_min"] = round(res["predict"]["min"] / res["module"]["min"], 4)
    res["logits_max_rel_difference"] = agree
    return res


def profile(model, bs):
    """per route one forward under the engine's per-launch events: {kernel: [launches, ms, algorithmic MB]}"""
    eng = model.engine()
    x = torch.randn((bs, 3, 224, 224), generator=torch.Generator().manual_seed(0)).cuda()
    out = {}
    with torch.no_grad():
        for name, fn in (("module", lambda: model(x)), ("predict", lambda: model.fused_predict(x))):
            fn()
            rows = {}
            for rep in range(5):        # summed over 5 forwards, reported per forward
                eng.profile_gemms(fn, all_kernels=True)
                for k, (n, ms, fl, by) in eng.last_profile_by_shape.items():
                    key = f"gemm {EPI_NAMES.get(k[0], k[0])} M={k[1]} N={k[2]} K={k[3]}"
                    e = rows.setdefault(key, [0, 0.0, 0.0]); e[0] += n; e[1] += ms; e[2] += by
                for k, (n, ms, by) in eng.last_profile_hbm.items():
                    e = rows.setdefault(k, [0, 0.0, 0.0]); e[0] += n; e[1] += ms; e[2] += by
            out[name] = {k: {"launches": v[0] // 5, "us": round(v[1] / 5 * 1e3, 1), "algorithmic_MB": round(v[2] / 5 / 1e6, 2)}
                         for k, v in sorted(rows.items())}
            out[name]["TOTAL"] = {"us": round(sum(v[1] for v in rows.values()) / 5 * 1e3, 1),
                                  "algorithmic_MB": round(sum(v[2] for v in rows.values()) / 5 / 1e6, 2)}
    return out


def rule_of(method, seed=11):
    """Compacter's frozen (4,4,4) rule, which the synthetic state dict leaves zero; None for the other methods"""
    return torch.rand((4, 4, 4), generator=torch.Generator().manual_seed(seed)) * 2 - 1 if method == "compacter" else None


def serving_sizes(lib, method="kadaptation"):
    """arena / workspace bytes of the training and the inference-only context, from the size queries (no allocation)"""
    import ctypes as C
    from pevit_amd import _lib
    from pevit_amd.synth import ARCHS
    out = {}
    for name in ("ViT-B/32", "ViT-B/16", "ViT-L/14"):
        a = ARCHS[name]
        d = _lib.PevitDims(a.width, a.layers, a.patch, a.resolution, a.embed_dim, _lib.METHOD_IDS[method], 4, 100, _lib.WEIGHT_FORMATS["bf16"])
        row = {}
        for kind, creator in (("train", "pevit_ctx_create"), ("serving", "pevit_infer_create")):
            if not hasattr(lib, creator):
                continue
            ctx = C.c_void_p()
            _lib.check(getattr(lib, creator)(C.byref(d), C.byref(ctx)), creator)
            row[kind] = {"arena_bytes": lib.pevit_arena_bytes(ctx), "workspace_bytes_bs32": lib.pevit_workspace_bytes(ctx, 32),
                         "workspace_bytes_bs128": lib.pevit_workspace_bytes(ctx, 128)}
            lib.pevit_ctx_destroy(ctx)
        out[name] = row
    return out


def serving_leg(steps, reps, route, method="kadaptation"):
    from pevit_amd import _lib
    from pevit_amd.engine import HipEngine, adapter_param_spec
    from pevit_amd.synth import ARCHS, randomize_adapters, synth_state_dict
    dev = torch.device("cuda", 0)
    arch, classes = ARCHS["ViT-B/32"], 100
    sd = {k: v for k, v in synth_state_dict(arch, seed=2, text_tower=False).items() if k.startswith("visual.")}
    ad = [(n, torch.zeros(s)) for n, s, _ in adapter_param_spec(method, arch.width, arch.layers)]
    randomize_adapters(ad, seed=3)
    sd.update(dict(ad))
    eng = HipEngine(arch, method, classes, 128)
    eng.load_state_dict(sd)
    rule = rule_of(method)
    if rule is not None:
        eng.load_phm_rule(rule)
    g = torch.Generator().manual_seed(5)
    v = eng.param_views()
    with torch.no_grad():
        v["layers.0.weight"].copy_(((torch.rand((classes, 512), generator=g) * 2 - 1) / 512 ** 0.5).cuda())
        eng.running_var.copy_((0.5 + torch.rand(512, generator=g)).cuda())
    routes, out = {}, {"method": method, "sizes": serving_sizes(eng.lib, method)}
    if route in ("both", "serving"):
        from pevit_amd import adapter_io
        from pevit_amd.serving import InferenceEngine
        ckpt = adapter_io.engine_adapter_state(eng, sd, phm_rule=rule)
        inf = InferenceEngine(arch, method, classes, 128)
        inf.load_backbone(sd)
        for name in ("a", "b"):
            inf.add_adapter(name, ckpt)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(2000):
            inf.use("ab"[i & 1])
        out["use_us"] = round((time.perf_counter() - t0) / 2000 * 1e6, 3)
        routes["serving"] = inf.predict
        out["bound"] = {"train": {"arena_bytes": eng.arena.numel(), "workspace_bytes": eng.workspace.numel()},
                        "serving": {"arena_bytes": inf.arena_bytes, "workspace_bytes": inf.workspace_bytes}}
    if route in ("both", "train"):
        routes["train"] = eng.predict
    else:
        del eng
        torch.cuda.empty_cache()
    for bs in (128, 32):
        x = torch.randn((steps * bs, 3, 224, 224), generator=torch.Generator().manual_seed(0)).to(dev)
        batches = [x[i * bs:(i + 1) * bs] for i in range(steps)]
        if len(routes) == 2:
            out[f"bs{bs}_bit_identical"] = bool(torch.equal(routes["train"](batches[0]), routes["serving"](batches[0])))
        for r in routes.values():
            run_pass(r, batches)                                  # warm-up pass
        wall = {r: [] for r in routes}
        order = list(routes)
        for rep in range(reps):
            for r in (order if rep % 2 == 0 else order[::-1]):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                run_pass(routes[r], batches)
                torch.cuda.synchronize(dev)
                wall[r].append(round(steps * bs / (time.perf_counter() - t0), 1))
        out[f"bs{bs}_images_per_s_rounds"] = wall
        del x, batches
    return out


def segments_leg(steps, reps, one_pass=None, method="kadaptation"):
    """ViT-B/32 + ``method``, 8 resident adapters, 8 requests of 16 images for 8 different adapters: the loop ``use(name);
    predict(images)`` per request on a plain context ("loop": the route before segments, unchanged code) against one
    ``predict_segments`` call on a ``slots = 8`` context ("segments"), same images, passes in alternation as the other legs.  Next
    to it what a ``slots = 8`` context costs: ``predict`` at batch 128 on it against the plain context (its QKV product is 512
    columns wider than 3 E + 64 for the single-adapter calls; a post-MLP slot context runs the very launches of the plain one), and
    the arena / workspace bytes of both."""
    from pevit_amd import adapter_io
    from pevit_amd.engine import HipEngine, adapter_param_spec
    from pevit_amd.serving import InferenceEngine
    from pevit_amd.synth import ARCHS, randomize_adapters, synth_state_dict
    dev = torch.device("cuda", 0)
    arch, classes, n_req, req = ARCHS["ViT-B/32"], 100, 8, 16
    sd = {k: v for k, v in synth_state_dict(arch, seed=2, text_tower=False).items() if k.startswith("visual.")}
    ckpts = []
    for i in range(n_req):                                # eight different adapters and heads
        ad = [(n, torch.zeros(s)) for n, s, _ in adapter_param_spec(method, arch.width, arch.layers)]
        randomize_adapters(ad, seed=3 + i)
        eng = HipEngine(arch, method, classes, 16)
        eng.load_state_dict(dict(sd, **dict(ad)))
        rule = rule_of(method, seed=11 + i)                 # (Compacter: eight different frozen rules too)
        if rule is not None:
            eng.load_phm_rule(rule)
        g = torch.Generator().manual_seed(5 + i)
        with torch.no_grad():
            eng.param_views()["layers.0.weight"].copy_(((torch.rand((classes, 512), generator=g) * 2 - 1) / 512 ** 0.5).cuda())
            eng.running_var.copy_((0.5 + torch.rand(512, generator=g)).cuda())
        ckpts.append(adapter_io.engine_adapter_state(eng, sd, phm_rule=rule))
        del eng
    torch.cuda.empty_cache()
    names = [f"task{i}" for i in range(n_req)]
    engines = {}
    for kind, slots in (("plain", 1), ("slots8", 8)):
        e = InferenceEngine(arch, method, classes, 128, slots=slots)
        e.load_backbone(sd)
        for n, ck in zip(names, ckpts):
            e.add_adapter(n, ck)
        engines[kind] = e
    plain, multi = engines["plain"], engines["slots8"]
    out = {"method": method, "sizes": {k: {"arena_bytes": e.arena_bytes, "workspace_bytes_max_batch_128": e.workspace_bytes} for k, e in engines.items()}}
    x = torch.randn((steps, n_req * req, 3, 224, 224), generator=torch.Generator().manual_seed(0)).to(dev)

    def loop(batch):
        res = []
        for i, n in enumerate(names):
            plain.use(n)
            res.append(plain.predict(batch[i * req:(i + 1) * req]))
        return res

    def segments(batch):
        return multi.predict_segments([(n, batch[i * req:(i + 1) * req]) for i, n in enumerate(names)])

    def single128(e):
        def fn(batch):
            e.use(names[0])
            return e.predict(batch)
        return fn
    if one_pass:
        fn = {"loop": loop, "segments": segments}[one_pass]
        for i in range(steps):
            fn(x[i])
        torch.cuda.synchronize(dev)
        return {"one_pass": one_pass, "calls": steps}
    a, b = loop(x[0]), segments(x[0])
    torch.cuda.synchronize(dev)
    out["requests_bit_identical"] = [bool(torch.equal(p, q)) for p, q in zip(a, b)]
    # A request runs on 16 x 50 rows in the loop and among 128 x 50 in the segmented call: the row-wise GEMMs may be planned
    # differently.  The floor of that (tests/test_gpu_segments.py, test 4): the frozen tower alone, whole batch against its slices
    rel = lambda p, q: float((p.double() - q.double()).abs().max() / (q.double().abs().max() + 1e-30))
    out["requests_max_rel_distance"] = [rel(q, p) for p, q in zip(a, b)]
    # ... and that the plan is ALL they differ by: at the same row count a lone segment is predict bit for bit, and at the full
    # row count a request's answer does not depend on which adapters serve the other seven
    lone = multi.predict_segments([(names[0], x[0][:req])])[0]
    uniform = multi.predict_segments([(names[0], x[0][i * req:(i + 1) * req]) for i in range(n_req)])[0]
    torch.cuda.synchronize(dev)
    out["lone_segment_is_predict_bit_identical"] = bool(torch.equal(lone, a[0]))
    out["request_0_same_bits_whoever_shares_the_call"] = bool(torch.equal(uniform, b[0]))
    out["lone_segment_against_shared_call_max_rel"] = rel(b[0], lone)
    eng = HipEngine(arch, "none", classes, 16)
    eng.load_state_dict(sd)
    with torch.no_grad():
        eng.param_views()["layers.0.weight"].copy_(((torch.rand((classes, 512), generator=torch.Generator().manual_seed(4)) * 2 - 1) / 512 ** 0.5).cuda())
    none = InferenceEngine(arch, "none", classes, 128)
    none.load_backbone(sd)
    none.add_adapter("head", adapter_io.engine_adapter_state(eng, sd))
    none.use("head")
    whole = none.predict(x[0]).clone()
    out["plan_floor_method_none"] = max(rel(whole[i * req:(i + 1) * req], none.predict(x[0][i * req:(i + 1) * req])) for i in range(n_req))
    del eng, none
    for label, routes in (("requests_8x16", {"loop": loop, "segments": segments}),
                          ("predict_bs128", {"plain": single128(plain), "slots8": single128(multi)})):
        for r in routes.values():
            run_pass(r, x)                                        # warm-up pass
        wall = {r: [] for r in routes}
        order = list(routes)
        for rep in range(reps):
            for r in (order if rep % 2 == 0 else order[::-1]):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                run_pass(routes[r], x)
                torch.cuda.synchronize(dev)
                wall[r].append(round(steps * n_req * req / (time.perf_counter() - t0), 1))
        out[f"{label}_images_per_s_rounds"] = wall
        med = {r: statistics.median(v) for r, v in wall.items()}
        first, second = order
        out[f"{label}_{second}_over_{first}"] = round(med[second] / med[first], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--one-pass", choices=["module", "predict"], default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--serving", action="store_true")
    ap.add_argument("--serving-route", choices=["both", "train", "serving"], default="both")
    ap.add_argument("--segments", action="store_true")
    ap.add_argument("--segments-one-pass", choices=["loop", "segments"], default=None)
    ap.add_argument("--method", choices=["kadaptation", "lora", "adapter", "compacter"], default="kadaptation")
    args = ap.parse_args()
    if args.segments or args.segments_one_pass:
        s = json.dumps(segments_leg(args.steps, args.reps, args.segments_one_pass, args.method), indent=1)
        print(s)
        if args.out:
            with open(args.out, "w") as f:
                f.write(s + "\n")
        return
    if args.serving:
        s = json.dumps(serving_leg(args.steps, args.reps, args.serving_route, args.method), indent=1)
        print(s)
        if args.out:
            with open(args.out, "w") as f:
                f.write(s + "\n")
        return
    from pevit_amd.config import default_config
    from pevit_amd.evaluation import _harness
    from pevit_amd.synth import ARCHS, synth_state_dict
    arch = dataclasses.replace(ARCHS["ViT-B/32"], text_layers=1)
    test_bs = int(default_config().TEST.BATCH_SIZE_PER_GPU)
    out = {"how": f"ViT-B/32, synthetic weights, 100 classes, resident f32 images; a pass = {args.steps} batches; one warm-up pass per "
                  f"route, then {args.reps} timed passes per route in alternation; wall clock between two synchronises"}
    with tempfile.TemporaryDirectory() as tmp:
        ckpt = os.path.join(tmp, "vitb32_synth.pt")
        torch.save(synth_state_dict(arch, seed=2, text_tower=True), ckpt)
        if args.one_pass:
            model = build("kadaptation", ckpt, 128)
            x = torch.randn((128, 3, 224, 224), generator=torch.Generator().manual_seed(0)).cuda()
            fn = model.fused_predict if args.one_pass == "predict" else model
            with torch.no_grad():
                for _ in range(1 + args.steps):
                    fn(x)
            torch.cuda.synchronize()
            print(json.dumps({"one_pass": args.one_pass, "forwards": 1 + args.steps, "batch": 128}))
            return
        for method, sizes in (("kadaptation", (64, 128, test_bs)), ("adapter", (128,))):
            model = build(method, ckpt, 128)
            for bs in sizes:
                out[f"{method}_bs{bs}"] = measure(model, bs, args.steps, args.reps)
            if args.profile:
                out[f"{method}_bs128_per_kernel"] = profile(model, 128)
            del model
            _harness._BACKBONES.clear()
    s = json.dumps(out, indent=1)
    print(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
