#!/usr/bin/env python3
"""Workloads for the rocprofv3 kernel traces behind profiles/attn_seam.md (run under `rocprofv3 --kernel-trace --stats`).
usage: attn_seam_probe.py probs   -- attn_probs (head mean and per head) at the three tower geometries, 20 launches each
       attn_seam_probe.py seam    -- resblocks[0].attn forward (+ head-mean weights) and backward, ViT-B/32 KAdaptation, B = 128
       attn_seam_probe.py block   -- resblocks[0] forward and backward, same model and batch
The seam / block modes run two warm-up rounds first and then the traced round between two device synchronisations; the kernel
names of the last round are the launch list."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pevit_amd import _lib  # noqa: E402

GEOMETRIES = [("ViT-B/32", 128, 12, 50), ("ViT-B/16", 64, 12, 197), ("ViT-L/14", 32, 16, 257)]


def probs():
    lib = _lib.load()
    for name, B, H, N in GEOMETRIES:
        q = (torch.randn(B * H, N, 64, device="cuda") * 0.4).bfloat16()
        k = (torch.randn(B * H, N, 64, device="cuda") * 0.4).bfloat16()
        lse = torch.logsumexp(torch.bmm(q.float(), k.float().transpose(1, 2)), dim=-1).contiguous()
        for average in (1, 0):
            out = torch.empty((B, N, N) if average else (B, H, N, N), device="cuda")
            for _ in range(20):
                _lib.check(lib.pevit_op_attn_probs(_lib.stream_ptr(), _lib.ptr(q), _lib.ptr(k), _lib.ptr(lse), _lib.ptr(out), B, H, N,
                                                   average), "attn_probs")
        torch.cuda.synchronize()
        print(f"{name}: B={B} H={H} N={N} done")


def seam_or_block(mode):
    from pevit_amd.engine import HipEngine, adapter_param_spec
    from pevit_amd.synth import ARCHS, randomize_adapters, synth_state_dict
    arch, B = ARCHS["ViT-B/32"], 128
    sd = {k: v for k, v in synth_state_dict(arch, seed=2, text_tower=False).items() if k.startswith("visual.")}
    ad = [(n, torch.zeros(s)) for n, s, _ in adapter_param_spec("kadaptation", arch.width, arch.layers)]
    randomize_adapters(ad, seed=3)
    sd.update(dict(ad))
    eng = HipEngine(arch, "kadaptation", 10, B)
    eng.load_state_dict(sd)
    x = torch.randn(arch.tokens, B, arch.width, device="cuda")
    dy = torch.randn(arch.tokens, B, arch.width, device="cuda")
    for _ in range(3):
        torch.cuda.synchronize()
        if mode == "seam":
            eng.attention_forward(x, 0, weights="mean")
            eng.attention_backward(dy, 0)
        else:
            eng.blocks_forward(x, 0, 1)
            eng.blocks_backward(dy, 0, 1)
        torch.cuda.synchronize()
    print(f"{mode} done")


if __name__ == "__main__":
    probs() if sys.argv[1] == "probs" else seam_or_block(sys.argv[1])
