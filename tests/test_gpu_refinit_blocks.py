"""The ill-conditioned adapter gradients at the reference initialisation, gated PER TENSOR, one block at a time.

tests/test_gpu_refinit.py runs the towers free and has to leave the down path of the two post-MLP adapters (LayerNorm affine, down
projection and its bias; after five steps most Compacter tensors) without a per-tensor gate: 132 of 222 recorded Adapter tensors, 96
of 294 Compacter tensors.  Those tensors are what the fused post-MLP backward (adapter_fused.hip) with tn_gemm64, ln_bwd_affine,
colsum_reduce and chain_adapter / chain_compacter (adapter.hip) produce, and one of them zeroed, sign-flipped or short of one row
chunk in one block could pass the suite.

Here every block l of the full-size tower runs ALONE through the (N,B,E) seam (blocks_forward / zero_grad / blocks_backward over
[l, l + 1)), at the fixture's state -- step 0 and after four emulated SGD steps -- on exactly the input x_l and upstream gradient dy_l
that the CPU emulation oracle/emul_bf16.py sees at that block (tests/test_refinit_blocks_host.py: fixture_state, capture_block_io,
block_reference, gates; its CPU tests show that every gate stays below 0.95 and that a zeroed, negated, permuted or three-images-short
tensor fails it).  Asserted per block: y, dx and every gradient tensor against the emulation at

    max( existing gate of tests/test_gpu_emulation.py,  1.5 x how far plain f32 arithmetic is from the emulation on this kind )

gradients the emulation leaves None or exactly zero are exactly zero, gradients of every other block stay exactly zero.  Per case:
every gate is below 0.95, every trainable tensor with a non-zero emulated gradient was compared, and the MEDIAN over the tensors whose
own yardstick exceeds their existing gate of (engine error / the tensor's own yardstick) is at most 1.5 -- a systematic loss of
accuracy shows there before a single tensor fails.  On f32-verify (f32 storage and contractions, the same launch sequences) the
reference is ref_cpu.block_forward on the same inputs and every tensor is held to the stated 5e-2: arithmetic apart from layout.

Each case prints its record -- per kind the worst engine error, the yardstick and the gate; the median and the largest ratio -- and,
with PEVIT_RECORD_DIR=<dir> set, writes it to <dir>/refinit_blocks/<fixture>_<steps>_<format>.json.

The captured inputs are themselves a draw of the chaos this file conditions away -- the emulated tower runs free up to block l, and
for four steps before that -- so the yardstick of the worst block moves with the HOST's summation order (bottleneck Adapter down-path
biases, seen on two hosts at 4, 8 and 16 CPU threads: 0.24 to 0.53 after 4 steps, 0.27 to 0.36 at step 0).  The gates follow, since
they are computed from the very inputs the engine is then given; the widest seen is 0.80.

Measured on an MI355X (one run; worst block of each kind: engine error / the kind's yardstick, i.e. the gate is at 1.5):

    case                      y     dx    down path (LN affine, down weight(s), down bias)   up weight(s)   up bias    median / max
    Adapter B/32    step 0    0.27  0.18  0.10-0.14  (engine 3.6-4.0e-2, yardstick 0.27-0.36)  0.51         5e-6       0.05 / 0.66
    Adapter B/32    4 steps   0.27  0.36  0.44-0.60  (engine 0.17-0.29,  yardstick 0.37-0.48)  0.58         5e-6       0.05 / 0.99
    Compacter B/16  step 0    0.41  0.55  0.20-0.38  (engine 2.5-3.9e-2, yardstick 0.09-0.15)  0.38-0.48    8e-6       0.34 / 1.00
    Compacter B/16  4 steps   0.41  0.62  0.20-0.33  (engine 3.1-4.5e-2, yardstick 0.12-0.20)  0.32-0.43    2e-5       0.34 / 0.65
    LoRA r=8 B/32   step 0    0.23  0.26  adapter2 0.28-0.43 (adapter1 exactly zero)                                    - (no yardstick above
    LoRA r=8 B/32   4 steps   0.27  0.38  adapter1 0.41-0.46, adapter2 0.31-0.33                                           an existing gate)
    KAdaptation     4 steps   0.23  0.26  attn.b 0.42 (every Kronecker and rule factor exactly zero)                     -
    f32-verify, 4 steps       Adapter: y, dx 3e-7, gradients 3-7e-6; Compacter: y, dx 1e-6, gradients 0.8-6.5e-5  (gate 5e-2)

"median / max" is over the single tensors whose own yardstick exceeds their existing gate (37-43 of 96 Adapter, 101-103 of 120
Compacter tensors), each against its OWN yardstick; the median is asserted at 1.5.  The up bias is a plain column sum of the f32
upstream gradient on both sides: the engine reproduces it to 1e-6 while f32 arithmetic upstream of it is 0.11-0.26 away.  The one
place the engine comes near its yardstick is the Adapter's block 5 after four steps, where the cancellation is also strongest (that
blocks 4 and 5 set the yardstick, 0.29-0.48 against a median of 0.05-0.08 over the blocks).  Traced (profiles/refinit_blocks.md): it
is ONE ReLU mask bit.  With T = 400 < E the difference of the two down-weight gradients has a unique expansion sum_t c[t, j] z[t, :]
over the token rows; in block 5 a single (t, j) carries 99.4 % of the energy of c, the emulated pre-activation there is 3e-4 of the
median magnitude -- within round-off of zero, the mechanism behind RELU_PATH_TOL -- and the same c reproduces the difference of the
down biases to 9e-4.  One channel of that bias is off by 2.3 x the tensor's rms, the next by 0.05, the median channel by exactly 0.
(Compacter, whose gelu_new has no mask, stays at 0.2-0.4 in every block.)
"""
import json
import os

import pytest
import torch

from conftest import kind_of, rel_err
from test_gpu_refinit import PER_TENSOR_CAP, STATED_GRADS
from test_refinit_blocks_host import YARDSTICK_C, block_names, case, gated_tensors, is_zero, tensors_of

pytestmark = pytest.mark.gpu

CASES = [  # fixture, steps, weight format; cases on the same (fixture, steps) are adjacent: they share the cached CPU reference
    ("full_b32_adapter_refinit", 0, "bf16"), ("full_b32_adapter_refinit", 4, "bf16"), ("full_b32_adapter_refinit", 4, "f32-verify"),
    ("full_b16_compacter_refinit", 0, "bf16"), ("full_b16_compacter_refinit", 4, "bf16"), ("full_b16_compacter_refinit", 4, "f32-verify"),
    ("full_b32_lora_r8_refinit", 0, "bf16"), ("full_b32_lora_r8_refinit", 4, "bf16"),
    ("full_b32_kadaptation_refinit", 4, "bf16")]         # KAdaptation at step 0: test_reference_init_gives_bias_only_gradients


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def engine_at(state, weight_format):
    from pevit_amd.engine import HipEngine
    meta = state.meta
    eng = HipEngine(state.arch, meta["method"], meta["classes"], meta["batch"], lora_rank=meta["lora_r"], weight_format=weight_format)
    eng.load_state_dict(state.params)
    v = eng.param_views()
    with torch.no_grad():
        v["layers.0.weight"].copy_(state.head_w); v["layers.0.bias"].copy_(state.head_b)
    return eng


@pytest.mark.parametrize("tag,steps,weights", CASES, ids=[f"{t}-{s}-{w}" for t, s, w in CASES])
def test_every_block_alone_meets_its_gates(tag, steps, weights):
    c = case(tag, steps)
    f32 = weights == "f32-verify"
    eng = engine_at(c.state, weights)
    worst, ratios, failed, n_gated = {}, [], [], 0
    for l, ((x, dy), (em, plain)) in enumerate(zip(c.io, c.refs)):
        y = eng.blocks_forward(x.cuda(), l, l + 1)
        eng.zero_grad()
        dx = eng.blocks_backward(dy.cuda(), l, l + 1)
        torch.cuda.synchronize()
        flat = eng.grads.clone()
        got = {k: v.cpu() for k, v in eng.param_views(flat).items() if k in em.grads}
        got.update(y=y.cpu(), dx=dx.cpu())
        assert all(bool(torch.isfinite(v).all()) for v in got.values()), l
        for k in em.grads:                                                # what is left belongs to other blocks, or to the head
            eng.param_views(flat)[k].zero_()
        assert float(flat.abs().max()) == 0.0, (l, "a gradient outside the block was written")
        assert sorted(em.grads) == sorted(block_names(c.state, l))
        ref, own = tensors_of(plain if f32 else em), tensors_of(plain)
        for name, e in {"y": em.y, "dx": em.dx, **em.grads}.items():
            if is_zero(e):                                                # dead in the reference: exactly zero on the engine
                assert float(got[name].abs().max()) == 0.0, (l, name)
                continue
            kind = kind_of(name)
            gate, yard, existing = c.gates[kind]
            gate = STATED_GRADS if f32 else gate
            err = rel_err(got[name], ref[name])
            n_gated += 1
            w = worst.setdefault(kind, {"engine": 0.0, "block": l, "yardstick": yard, "gate": gate, "existing": existing})
            if err >= w["engine"]:
                w["engine"], w["block"] = err, l
            mine = rel_err(own[name], e)                                  # this tensor's own yardstick
            if not f32 and mine > existing:
                ratios.append(err / mine)
            if not err <= gate:
                failed.append((l, name, err, gate))
    ratios.sort()
    median = ratios[len(ratios) // 2] if ratios else 0.0
    rec = {"fixture": tag, "steps": steps, "weights": weights, "reference": "ref_cpu.block_forward" if f32 else "emul_bf16.block",
           "kinds": worst, "n_gated": n_gated, "ratio_to_own_yardstick": {"median": median, "max": ratios[-1] if ratios else 0.0, "n": len(ratios)},
           "kind_ratio_to_yardstick": {k: w["engine"] / w["yardstick"] for k, w in worst.items() if w["yardstick"] > w["existing"]}}
    print("refinit blocks:", json.dumps(rec))
    if os.environ.get("PEVIT_RECORD_DIR"):
        out = os.path.join(os.environ["PEVIT_RECORD_DIR"], "refinit_blocks")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, f"{tag}_{steps}_{weights}.json"), "w") as f:
            json.dump(rec, f, indent=1)
    assert not failed, failed[:8]
    assert all(g[0] < PER_TENSOR_CAP for g in c.gates.values()), c.gates
    assert n_gated == len(gated_tensors(c)) > 0 and sorted(worst) == sorted(c.gates)       # nothing skipped
    assert median <= YARDSTICK_C, (median, ratios[-8:])
