"""Input-resize rates on the engine (uint8 pixels at their native size -> the tower's 224 x 224, csrc/resize.hip).

  kernel   microseconds per pevit_resize_u8 launch at B = 128 (384 planes) for 32 -> 224, 96 -> 224 and 448 -> 224, HIP events over
           --iters back-to-back launches, next to the launch's byte floor: (source + destination bytes) / the HBM peak.
  harness  images/s of the reference-API path (train_one over a synthetic uint8 TensorLoader, ViT-B/32 + KAdaptation, batch 128,
           --steps full batches, the epoch-end read-back included) for four legs: the set pre-resized to 224 x 224, and the set at its
           native 32 x 32 with the engine's resize -- each resident on the GPU and host-fed (pinned staging, one batch ahead).  With
           it: the bytes a host-fed batch uploads and the bytes the image set occupies.

Every leg runs one warm-up, then --rounds timed rounds in alternation; wall clock is taken between synchronises.
--ragged: the ragged kernel (csrc/resize_ragged.hip: pevit_resize_ragged_u8) instead -- a uniform 32 x 32 set and a uniform 96 x 96
set of B = 128 images, timed against pevit_resize_u8 on the same pixels in alternation (the ragged kernel adds one descriptor read per
workgroup and nothing per pixel, so its median should lie inside the dense kernel's own min-max spread), and one mixed-size batch
(sides drawn in [96, 448], seeded): microseconds, and its bytes against the byte floor.
--one-pass SIZE: nothing but --iters launches of the kernel at that source size (the process to put under
rocprofv3 --kernel-trace --stats).
Prints one JSON object.  usage: python scripts/resize_rate.py [--rounds 3] [--iters 200] [--steps 20] [--one-pass SIZE] [--skip-harness] [--ragged] [--out FILE]"""
import argparse
import ctypes as C
import dataclasses
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12          # bytes/s, MI355X (8 HBM3E stacks)
B, N_PX, SIZES = 128, 224, (32, 96, 448)


def sync():
    torch.cuda.synchronize()


class KernelCase:
    """one source size: device tables from the library's planner, a random source batch and a destination"""

    def __init__(self, lib, size):
        from pevit_amd import _lib
        self.lib, self.size = lib, size
        nh, nw, top, left = (C.c_int() for _ in range(4))
        _lib.check(lib.pevit_resize_geometry(size, size, N_PX, C.byref(nh), C.byref(nw), C.byref(top), C.byref(left)), "geometry")
        self.t = []
        for in_size, out_size, first in ((size, nw.value, left.value), (size, nh.value, top.value)):
            ks = lib.pevit_resize_axis(in_size, out_size, 0, 0, None, None)
            k, b = torch.empty((N_PX, ks), dtype=torch.int32), torch.empty((N_PX, 2), dtype=torch.int32)
            _lib.check(lib.pevit_resize_axis(in_size, out_size, first, N_PX, C.c_void_p(k.data_ptr()), C.c_void_p(b.data_ptr())), "axis")
            self.t += [k.cuda(), b.cuda(), ks]
        self.src = torch.randint(0, 256, (B, 3, size, size), dtype=torch.uint8, generator=torch.Generator().manual_seed(size)).cuda()
        self.dst = torch.empty((B, 3, N_PX, N_PX), dtype=torch.uint8, device="cuda")
        self.bytes = self.src.numel() + self.dst.numel()

    def launch(self):
        from pevit_amd import _lib
        kh, bh, ksh, kv, bv, ksv = self.t
        _lib.check(self.lib.pevit_resize_u8(_lib.stream_ptr(), _lib.ptr(self.src), 3 * B, self.size, self.size, _lib.ptr(self.dst),
                                            N_PX, N_PX, _lib.ptr(kh), _lib.ptr(bh), ksh, _lib.ptr(kv), _lib.ptr(bv), ksv), "pevit_resize_u8")

    def us_per_launch(self, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            self.launch()
        e1.record()
        sync()
        return e0.elapsed_time(e1) * 1e3 / iters


def kernel_rates(lib, rounds, iters):
    cases = [KernelCase(lib, s) for s in SIZES]
    for c in cases:
        c.us_per_launch(20)                                # warm-up
    out = {f"{c.size}->224": {"us": [], "bytes": c.bytes, "floor_us": c.bytes / HBM_PEAK * 1e6} for c in cases}
    for _ in range(rounds):
        for c in cases:
            out[f"{c.size}->224"]["us"].append(round(c.us_per_launch(iters), 3))
    for v in out.values():
        v["floor_share"] = round(v["floor_us"] / min(v["us"]), 4)
    return out


class RaggedCase:
    """a ragged set of B images on the device (preprocess.RaggedImages, tables from the library's planner) and a destination"""

    def __init__(self, lib, shapes, seed):
        import numpy as np
        from pevit_amd import _lib
        from pevit_amd.preprocess import RaggedImages, ragged_offsets
        self.lib = lib
        g = np.random.default_rng(seed)
        pool = g.integers(0, 256, int(ragged_offsets(shapes)[-1]), dtype=np.uint8)
        self.set = RaggedImages.build(pool, shapes, N_PX, True).to("cuda")
        self.dst = torch.empty((len(shapes), 3, N_PX, N_PX), dtype=torch.uint8, device="cuda")
        self.bytes = self.set.pool.numel() + self.dst.numel()
        r = self.set
        self.args = _lib.PevitResizeRaggedArgs(
            pool=_lib.ptr(r.pool), pool_bytes=r.pool.numel(), desc=_lib.ptr(r.desc), k_pool=_lib.ptr(r.k_pool), k_len=r.k_pool.numel(),
            b_pool=_lib.ptr(r.b_pool), b_len=r.b_pool.numel(), index=None, dst=_lib.ptr(self.dst), n_images=len(r), batch=len(r),
            out=N_PX, max_ksize_v=r.max_ksize_v)

    def launch(self):
        from pevit_amd import _lib
        _lib.check(self.lib.pevit_resize_ragged_u8(_lib.stream_ptr(), C.byref(self.args)), "pevit_resize_ragged_u8")

    us_per_launch = KernelCase.us_per_launch


def _spread(us):
    s = sorted(us)
    return {"us": us, "median": s[len(s) // 2], "min": s[0], "max": s[-1]}


def ragged_rates(lib, rounds, iters):
    """uniform sets: the ragged kernel against the dense one on the same pixels, in alternation; then one mixed-size batch"""
    import numpy as np
    out = {}
    for size in (32, 96):
        dense, ragged = KernelCase(lib, size), RaggedCase(lib, [(size, size)] * B, size)
        ragged.set.pool.copy_(dense.src.reshape(-1))                 # the same pixels
        dense.launch(); ragged.launch(); sync()
        assert torch.equal(dense.dst, ragged.dst), "the ragged kernel's bytes differ from the dense kernel's"
        dense.us_per_launch(20); ragged.us_per_launch(20)            # warm-up
        d, r = [], []
        for _ in range(rounds):
            d.append(round(dense.us_per_launch(iters), 3)); r.append(round(ragged.us_per_launch(iters), 3))
        out[f"uniform_{size}->224"] = {"dense": _spread(d), "ragged": _spread(r), "bytes": dense.bytes,
                                        "ragged_median_inside_dense_spread": bool(min(d) <= _spread(r)["median"] <= max(d))}
    shapes = np.random.default_rng(0).integers(96, 449, (B, 2)).tolist()
    mixed = RaggedCase(lib, [tuple(s) for s in shapes], 1)
    mixed.us_per_launch(20)
    us = [round(mixed.us_per_launch(iters), 3) for _ in range(rounds)]
    out["mixed_96..448->224"] = dict(_spread(us), bytes=mixed.bytes, floor_us=mixed.bytes / HBM_PEAK * 1e6,
                                      floor_share=round(mixed.bytes / HBM_PEAK * 1e6 / min(us), 4), max_ksize_v=mixed.set.max_ksize_v,
                                      table_bytes=mixed.set.table_bytes)
    return out


def harness_rates(rounds, steps, native=32):
    from pevit_amd.config import vitb32_clip_config
    from pevit_amd.evaluation import kadaptation_clip as mod
    from pevit_amd.evaluation.dataloader import TensorLoader, _Tensors
    from pevit_amd.optim import build_optimizer
    from pevit_amd.preprocess import resize_center_crop_u8
    from pevit_amd.synth import ARCHS, synth_state_dict
    arch = dataclasses.replace(ARCHS["ViT-B/32"], text_layers=1)
    dev = torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as tmp:
        ckpt = os.path.join(tmp, "vitb32_synth.pt")
        torch.save(synth_state_dict(arch, seed=2, text_tower=True), ckpt)
        cfg = vitb32_clip_config()
        cfg.MODEL.NAME = ckpt
        cfg.DATASET.NUM_CLASSES = 100
        cfg.TRAIN.LR, cfg.TRAIN.WD = 0.01, 1e-6
        cfg.TRAIN.BATCH_SIZE_PER_GPU = cfg.TEST.BATCH_SIZE_PER_GPU = B
        cfg.GPUS = (0,)
        model = mod.Classifier(cfg, 0).cuda(dev)
        crit = torch.nn.CrossEntropyLoss()
        opt = build_optimizer(cfg, model)
        assert model.can_fuse(crit, opt)
        g = torch.Generator().manual_seed(0)
        n = steps * B
        small = torch.randint(0, 256, (n, 3, native, native), dtype=torch.uint8, generator=g)
        big = resize_center_crop_u8(small, N_PX)              # the same pictures, resized offline
        labels = torch.randint(0, 100, (n,), generator=g)
        legs = {"pre_resized_224_resident": (big.to(dev), labels.to(dev)), f"native_{native}_resident": (small.to(dev), labels.to(dev)),
                "pre_resized_224_host_fed": (big, labels), f"native_{native}_host_fed": (small, labels)}
        loaders = {k: TensorLoader(_Tensors(*v), batch_size=B, shuffle=True) for k, v in legs.items()}
        out = {k: {"images_per_s": [], "set_bytes": v[0].numel(), "bytes_per_batch": B * v[0][0].numel()} for k, v in legs.items()}
        for k, loader in loaders.items():
            mod.train_one(loader, model, crit, opt, 0, cfg)       # warm-up epoch (staging buffers, tables)
        sync()
        for r in range(rounds):
            for k, loader in loaders.items():
                sync()
                t0 = time.perf_counter()
                mod.train_one(loader, model, crit, opt, 1 + r, cfg)
                sync()
                out[k]["images_per_s"].append(round(n / (time.perf_counter() - t0), 1))
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--one-pass", type=int, default=0)
    ap.add_argument("--skip-harness", action="store_true")
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from pevit_amd import _lib
    lib = _lib.load()
    torch.cuda.set_device(0)
    if a.one_pass:
        c = KernelCase(lib, a.one_pass)
        for _ in range(a.iters):
            c.launch()
        sync()
        print(json.dumps({"one_pass": a.one_pass, "launches": a.iters}))
        return
    res = {"ragged": ragged_rates(lib, a.rounds, a.iters)} if a.ragged else {"kernel": kernel_rates(lib, a.rounds, a.iters)}
    if not a.skip_harness and not a.ragged:
        res["harness"] = harness_rates(a.rounds, a.steps)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
