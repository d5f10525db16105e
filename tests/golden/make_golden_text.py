#!/usr/bin/env python3
"""Text-tower fixtures (tests/golden/text_<tag>.npz / .json): ``encode_text`` of the imported REFERENCE CLIP in f32 on seeded tokens,
at widths the engine's text tower can run (make_golden.py's tiny_text.npz has text width 64).

Like make_golden.py this runs only where the reference is present; it needs no GPU.  The weights are not stored: they are
``synth_state_dict(VitArch(*arch), seed)`` rounded through fp16 as ``text_case()`` does, and the fixture holds the arch tuple, the
seed, the tokens, the reference's features and the zero-shot weights of the reference reduction (feature.py:513-520).

Each .json carries the bf16 floor measured on the reference itself, as the image fixtures do: the deviation of the reference's
features and zero-shot weights from its own f32 run with
  leg "weights":  the text block weights and text_projection rounded to bf16 (stored back as f32);
  leg "operands": the same, inside make_golden.bf16_operands (both operands of every contraction rounded to bf16).
No line of the engine is involved.

Usage:  python tests/golden/make_golden_text.py [tag ...]
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import FROZEN_BF16, bf16_operands, build_ref  # noqa: E402
from pevit_amd.synth import VitArch, synth_state_dict  # noqa: E402

SEED = 2
# tag -> (text width, layers, context, out_dim, vocab, prompts)
TAGS = {
    "w128_l2_n77": (128, 2, 77, 64, 512, 7),
    "w256_l3_n77": (256, 3, 77, 128, 512, 5),
    "w128_l2_n8": (128, 2, 8, 64, 32, 3),
    "w512_l12_n77": (512, 12, 77, 512, 1024, 64),      # the block shapes of ViT-B's text tower: 8 heads, E = 512; 4,928 rows
}


def text_arch(tag):
    """The smallest image tower the reference's build_model accepts next to the text tower under test."""
    width, layers, context, out_dim, vocab, _ = TAGS[tag]
    return VitArch("text-" + tag, 128, 1, 16, 32, out_dim, text_width=width, text_layers=layers, context_length=context,
                   vocab_size=vocab)


def arch_tuple(a):
    return [a.name, a.width, a.layers, a.patch, a.resolution, a.embed_dim, a.text_width, a.text_layers, a.context_length, a.vocab_size]


def class_sizes(prompts):
    """templates per class: 1, 3, 4 in turn while they fit (the reduction is tested with all three), the rest in one class"""
    sizes, left, turn = [], prompts, 0
    while left > 0:
        n = min((1, 3, 4)[turn % 3], left)
        sizes.append(n); left -= n; turn += 1
    return sizes


def seeded_tokens(tag):
    _, _, N, _, V, S = TAGS[tag]
    g = torch.Generator(device="cpu"); g.manual_seed(11)
    tokens = torch.randint(1, V - 1, (S, N), generator=g)
    eot = torch.randint(1, N, (S,), generator=g)
    # the end-of-text marker (the arg-max token, model.py:1166): at the last position, at position 0, on both sides of a 16-query
    # tile boundary (where the context is long enough), and twice in one prompt -- the FIRST occurrence must win
    edge = [N - 1, 0] + ([15, 16] if N > 17 else [])
    for i, p in enumerate(edge):
        if i < S - 1:
            eot[i] = p
    for s in range(S):
        tokens[s, eot[s]] = V - 1
        tokens[s, eot[s] + 1:] = 0
    first, second = (20, 41) if N > 42 else (3, 5)
    tokens[S - 1] = torch.randint(1, V - 1, (N,), generator=g)
    tokens[S - 1, first] = V - 1
    tokens[S - 1, second] = V - 1
    tokens[S - 1, second + 1:] = 0
    return tokens


def reduce_classes(feats, sizes):
    cols, o = [], 0
    for n in sizes:
        e = feats[o:o + n]; o += n
        e = e / e.norm(dim=-1, keepdim=True)
        m = e.mean(dim=0)
        cols.append(m / m.norm())
    return torch.stack(cols, dim=1)


def rel(a, b):
    a = a.double().flatten(); b = b.double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def mrel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


def round_text_weights_(model):
    n = 0
    with torch.no_grad():
        for name, p in model.named_parameters():
            if (name.startswith("transformer.resblocks.") and name.endswith(FROZEN_BF16)) or name == "text_projection":
                p.copy_(p.bfloat16().float()); n += 1
    return n


def text_fixture(tag):
    arch = text_arch(tag)
    sizes = class_sizes(TAGS[tag][5])
    tokens = seeded_tokens(tag)
    runs = {}
    for leg in (None, "weights", "operands"):
        torch.manual_seed(0)
        sd = synth_state_dict(arch, seed=SEED, text_tower=True)
        sd = {k: (v.half().float() if v.dim() > 0 else v) for k, v in sd.items()}
        model = build_ref("kadaptation", sd)
        if leg is not None:
            assert round_text_weights_(model) == 4 * arch.text_layers + 1
        with torch.no_grad():
            if leg == "operands":
                with bf16_operands(model):
                    feats = model.encode_text(tokens).float().clone()
            else:
                feats = model.encode_text(tokens).float().clone()
        runs[leg] = (feats, reduce_classes(feats, sizes))
        del model
    feats, zs = runs[None]
    floor = {"recipe": "tests/golden/make_golden_text.py: the imported reference's encode_text with (weights) the text block weights and "
                       "text_projection rounded to bf16, (operands) additionally both operands of every contraction rounded to bf16 "
                       "(make_golden.bf16_operands); deviation from the reference's own f32 run: max_rel = max abs / max abs of the "
                       "f32 run, rel_err = relative L2"}
    for leg in ("weights", "operands"):
        f, z = runs[leg]
        floor[leg] = {"max_rel": mrel(f, feats), "rel_err": rel(f, feats), "zeroshot_max_rel": mrel(z, zs), "zeroshot_rel_err": rel(z, zs)}
    meta = {"tag": tag, "arch": arch_tuple(arch), "seed": SEED, "fp16_rounded": True, "prompts": int(tokens.shape[0]),
            "class_sizes": sizes, "floor": floor}
    np.savez_compressed(os.path.join(HERE, f"text_{tag}.npz"), tokens=tokens.numpy(), text_features=feats.numpy(),
                        zeroshot_weights=zs.numpy())
    with open(os.path.join(HERE, f"text_{tag}.json"), "w") as fh:
        json.dump(meta, fh, indent=1)
    print(tag, "eot", tokens.argmax(dim=-1).tolist()[:8], "floor",
          {leg: "%.3g / %.3g" % (floor[leg]["max_rel"], floor[leg]["rel_err"]) for leg in ("weights", "operands")}, flush=True)


def main():
    torch.set_num_threads(8)
    for tag in (sys.argv[1:] or list(TAGS)):
        text_fixture(tag)


if __name__ == "__main__":
    main()
