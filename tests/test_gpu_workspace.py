"""No engine call reads workspace it did not write itself.

The activation workspace (``eng.workspace``) is shared by every call on a context, carved afresh for the batch of each call
(``layout_workspace`` in csrc/ctx.hip) and allocated with ``torch.empty``; only its leading flag region
(``pevit_workspace_state_bytes``: the stream-K hand-off flags, the error word, the skipped-update counter) carries state from one
launch to the next.  ``poison(eng)`` asserts that this region is all zero and fills EVERY byte behind it -- the stream-K slabs
included -- with 0xFF, a NaN as f32, as bf16 and as e4m3.  It is used only where no saved forward is pending: before a whole call
or before the forward of a forward / backward pair, never between a forward and its backward.

1. ``test_the_poison_bites``: next to the helper, the proof that the comparison sees it -- one element of ONE slot that is known
   to be read (the saved input of block 0) changed between a forward and its backward, and the whole poison put where it must not
   go, are both reported.
2. ``test_every_entry_point_is_self_contained_under_poison``: two engines with identical weights, parameters and BatchNorm
   buffers run the same calls; P is poisoned before every call, Q never (it keeps the finite, right-sized leftovers of whatever
   ran before: the pair is shared by all calls of a case).  Every output and every piece of state must be finite and equal bit
   for bit, at the default knobs.
   Entry points: three ``train_step``s; ``forward_backward`` + ``sgd_step``; ``forward_backward`` + ``optimizer_step`` (Adam);
   the BCE step; the uint8 step with and without the input resize; ``visual_forward(save=True)`` + ``head_forward_backward`` +
   ``visual_backward``; ``visual_forward(save=False)``; ``transformer_forward`` / ``transformer_backward``; ``blocks_forward`` /
   ``blocks_backward`` on blocks [1, L), and one call per block and back (the per-block saved slots are the one region that is
   meant to carry state across calls: poison before the first forward only); ``attention_forward`` ("mean" and "heads"
   weights) / ``attention_backward``; the two
   ``pevit_visual_backward_part`` halves of the staged DP route (one process, no process group, stream-K left on);
   ``predict``, ``encode_image``, ``zeroshot``; ``probe_step`` / ``probe_predict``; a captured step with poison between replays.
   Cases: tiny-128 (N = 10, H = 2: the fused delta + attention form, both class-token shortcuts; ``max_batch`` 8), tiny-256
   (N = 17, H = 4: the two attention kernels, the fused post-MLP adapter kernels; ``max_batch`` 5) and tiny-n257 (N = 257: the
   N > 64 branch that zeroes ``w_dO``; patch 14: a padded patch matrix; ``max_batch`` 4), each with every method in bf16 and
   f32-verify and with kadaptation / lora / none in fp8 and fp8-act.
   Batches: ``max_batch`` and an odd batch below it (8 and 5, 5 and 3, 4 and 3): the second call sequence runs on a layout whose
   slots all sit elsewhere.  ``pevit_op_attn_delta_hpw`` does not depend on the batch and takes every B at H = 2, N = 10, and the
   planner's occupancy rule keeps the fused form for the few runs of B <= 8: no batch makes tiny-128 leave the fused form at the
   default knobs (the test asks and would use one that did).  The "two-kernel" batch therefore switches ``fused_attn_delta`` off on
   BOTH engines of the pair (kadaptation and lora, bf16 and fp8 -- where the fused form is planned at all), so that delta-add +
   attention run on the same engines, on the odd batch.
   Refused by construction (the test asserts the refusal and that it leaves the flags alone): fp8 and fp8-act with adapter and
   compacter (``pevit_ctx_create``, tests/test_workspace_host.py), ``attention_forward`` under fp8-act, ``probe_step`` /
   ``probe_predict`` on any method but "none".
3. ``test_one_context_walks_the_reference_call_order``: ONE engine (``max_batch`` 8) through train 8, train 5, predict 7,
   train 8, encode_image 3, zeroshot 8, train 2, probe_step, train 8, reset_run, train 6, ensure_batch(12), train 12, train 8 --
   a partial last batch, evaluation through the inference layout, the next epoch -- poisoned before every call, flags clear after
   every call, against one control engine per batch that was built with that ``max_batch`` and takes the walker's state before
   the call.  Every method on tiny-128 ("none": ``probe_step`` runs; elsewhere its refusal is asserted), adapter on tiny-256,
   kadaptation and adapter on tiny-n257.  ``test_a_backward_after_another_forward_is_refused``: ``visual_forward(save=True)`` at 8, another forward at 4,
   ``visual_backward`` at 8 raises with the "saved activations" message and touches neither ``grads`` nor the flags; the same
   after ``ensure_batch`` has bound a new workspace (``pevit_bind`` used to leave the saved forward valid: the backward ran on
   uninitialised memory).  ``test_the_head_alone_at_a_larger_batch_than_the_last_saving_forward``: ``head_forward_backward`` used
   to keep the layout of the last saving forward whatever its own batch, and a larger batch overran the head's slots into each
   other (every bit of dfeat wrong); it now lays the workspace out for its batch and gives the saved forward up.
4. ``test_text_tower_is_self_contained_under_poison``: ``TextEngine.encode`` on the tiny text tower, bf16 and f32-verify, whole
   and chunked.
"""
import ctypes as C
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

CLASSES = 10
MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
STEP = dict(lr=0.05, momentum=0.9, weight_decay=1e-3)


@pytest.fixture(scope="module", autouse=True)
def _gpu_and_cleanup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield
    _PAIRS.clear()
    inputs.cache_clear()


# ---- 1. the poison helper, and the proof that it bites --------------------------------------------------------------------------
def state_bytes(eng):
    """The leading bytes of the workspace that carry state between launches, as the library states them."""
    n = eng.lib.pevit_workspace_state_bytes(eng._ctx)
    assert 0 < n < eng.workspace.numel() and n % 4 == 0
    return n


def assert_flags_clear(eng):
    """Every launch leaves the stream-K flags zero; the error word and the skipped-update counter stay zero with them."""
    torch.cuda.synchronize(eng.device)
    words = eng.workspace[:state_bytes(eng)].view(torch.int32)
    left = words.nonzero().flatten().tolist()
    assert not left, f"flag region: words {left[:8]} hold {words[left[:8]].tolist()}"


def poison(eng):
    """Synchronise, require the flag region clear, fill everything behind it with 0xFF.  Only where no saved forward is pending."""
    assert_flags_clear(eng)
    eng.workspace[state_bytes(eng):].fill_(0xFF)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def differences(got, want):
    """What the comparison reports: the tensors of ``got`` that are not finite, and those that differ from ``want``'s in any bit."""
    assert list(got) == list(want)
    bad = []
    for k, a in got.items():
        b = want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if a.is_floating_point() and not bool(torch.isfinite(a).all()):
            bad.append(f"{k}: {int((~torch.isfinite(a)).sum())} of {a.numel()} not finite")
        elif not torch.equal(bits(a), bits(b)):
            d = (bits(a) != bits(b)).flatten().nonzero().flatten()
            bad.append(f"{k}: {d.numel()} of {a.numel()} differ, first at {int(d[0])}")
    return bad


def engine_state(e):
    torch.cuda.synchronize(e.device)
    s = {"params": e.params, "grads": e.grads, "momentum": e.momentum, "running_mean": e.running_mean, "running_var": e.running_var,
         "exp_avg_sq": e.exp_avg_sq if e.exp_avg_sq is not None else torch.zeros_like(e.params)}
    return {"state." + k: v.clone() for k, v in s.items()}


def build(arch_name, method, weight_format, max_batch):
    """tests/test_gpu_predict.py's synthetic engine (random non-zero adapters, head and running statistics), with the Compacter
    rule of tests/test_gpu_tower.py's _full_size_case (the synthetic state-dict leaves it zero) and the uint8 constants set."""
    from test_gpu_predict import make_engine
    arch, eng = make_engine(arch_name, method, max_batch, weight_format=weight_format, classes=CLASSES)
    if method == "compacter":
        from test_gpu_tower import _full_size_case
        eng.load_phm_rule(_full_size_case(arch_name, method, 4)[1]["visual.transformer.phm_rule"])
    eng.set_input_normalization(MEAN, STD)
    return arch, eng


_PAIRS = {}


def restore(e, init):
    """The state the engine was built with: fresh optimizer, no gradients, the initial parameters and BatchNorm buffers, default knobs."""
    e.reset_run()
    e.params.copy_(init[0]); e.running_mean.copy_(init[1]); e.running_var.copy_(init[2])
    e.set_input_resize(False)
    e.tune("fused_attn_delta", 1)


def pair(arch_name, method, weight_format, max_batch):
    """(arch, P, Q) with identical weights, parameters and BatchNorm buffers, in their initial state; one pair per case, so Q's
    workspace holds what the calls before left there."""
    key = (arch_name, method, weight_format, max_batch)
    if key not in _PAIRS:
        (arch, p), (_, q) = build(*key), build(*key)
        assert torch.equal(p.arena, q.arena) and torch.equal(p.params, q.params) and float(p.params.abs().max()) > 0
        assert torch.equal(p.running_mean, q.running_mean) and torch.equal(p.running_var, q.running_var)
        _PAIRS[key] = (arch, p, q, (p.params.clone(), p.running_mean.clone(), p.running_var.clone()))
    arch, p, q, init = _PAIRS[key]
    for e in (p, q):
        restore(e, init)
    return arch, p, q


@functools.lru_cache(maxsize=None)
def inputs(arch_name, B):
    """Everything the calls read for a batch of B, seeded, on the device, never written."""
    from pevit_amd.synth import ARCHS, synth_batch
    arch = ARCHS[arch_name]
    R, N, E, D = arch.resolution, arch.tokens, arch.width, arch.embed_dim
    g = torch.Generator().manual_seed(17 + B)
    d = types.SimpleNamespace(B=B)
    d.images, d.labels = synth_batch(B, R, CLASSES, seed_img=3, seed_lbl=4)
    d.targets = (torch.rand((B, CLASSES), generator=g) < 0.3).float()
    d.u8 = torch.randint(0, 256, (B, 3, R, R), generator=g, dtype=torch.uint8)
    d.u8_native = torch.randint(0, 256, (B, 3, R + 10, R + 23), generator=g, dtype=torch.uint8)
    d.x = torch.randn((N, B, E), generator=g)
    d.dy = torch.randn((N, B, E), generator=g) * 0.1
    d.text = torch.nn.functional.normalize(torch.randn((7, D), generator=g), dim=1).contiguous()
    d.feats = torch.randn((24, D), generator=g)
    d.flabels = torch.randint(0, CLASSES, (24,), generator=g)
    d.index = torch.randperm(24, generator=g)[:B].contiguous()
    for k, v in vars(d).items():
        if torch.is_tensor(v):
            setattr(d, k, v.cuda())
    return d


def test_the_poison_pattern_is_a_nan_in_every_storage_type():
    raw = torch.full((8,), 0xFF, dtype=torch.uint8, device="cuda")
    for dtype in (torch.float32, torch.bfloat16, torch.float8_e4m3fn):
        assert bool(torch.isnan(raw.view(dtype).float()).all()), dtype


def test_the_poison_bites():
    """The comparison must report (a) ONE element of one slot changed by a finite amount behind the engine's back -- the saved
    input of block 0, which LayerNorm backward reads, found in the workspace by its contents and written through the test's own
    view of ``eng.workspace`` between ``transformer_forward`` and ``transformer_backward`` -- and (b) the poison itself put between
    a forward and its backward, where it must never go.  Without either, the same calls agree."""
    arch, p, q = pair("tiny-128", "kadaptation", "bf16", 8)
    d = inputs("tiny-128", 8)

    def fwd_bwd(e, between):
        e.zero_grad()
        y = e.transformer_forward(d.x, save=True)
        torch.cuda.synchronize()
        between(e)
        dx = e.transformer_backward(d.dy)
        return {"y": y, "dx": dx, **engine_state(e)}

    def nudge_block0_input(e):
        rows = d.x.permute(1, 0, 2).contiguous().flatten()              # the engine's rows are batch-major
        ws = e.workspace.view(torch.float32)
        at = [int(i) for i in (ws == rows[0]).nonzero().flatten() if torch.equal(ws[int(i):int(i) + rows.numel()], rows)]
        assert len(at) == 1, at
        ws[at[0] + 5] += 0.5

    want = fwd_bwd(q, lambda e: None)
    assert differences(fwd_bwd(p, lambda e: None), want) == []
    nudged = differences(fwd_bwd(p, nudge_block0_input), want)
    assert any(s.startswith("dx:") and "differ" in s for s in nudged), nudged
    assert not any(s.startswith("y:") for s in nudged), nudged          # the forward had finished
    poisoned = differences(fwd_bwd(p, lambda e: e.workspace[state_bytes(e):].fill_(0xFF)), want)
    assert any("not finite" in s for s in poisoned), poisoned
    assert_flags_clear(p)


# ---- 2. every entry point, poisoned against not ----------------------------------------------------------------------------------
def _put(out, **tensors):
    for k, v in tensors.items():
        if v is not None:
            out[k] = v.clone()


def call_train3(e, d, pre):
    out = {}
    for i in range(3):                  # the first-step flag, then momentum
        pre()
        logits, loss = e.train_step(d.images, d.labels, **STEP)
        _put(out, **{f"logits{i}": logits, f"loss{i}": loss})
    return out


def call_fb_sgd(e, d, pre):
    out = {}
    pre()
    logits, loss = e.forward_backward(d.images, d.labels)
    _put(out, logits=logits, loss=loss, grads_before_update=e.grads)
    pre()
    e.sgd_step(**STEP)
    return out


def call_fb_adam(e, d, pre):
    from pevit_amd.engine import OptimPlan
    group_of = torch.where(e.grad_mask_host.bool(), 0, 255).to(torch.uint8)
    plan = OptimPlan("adam", [dict(lr=1e-3, weight_decay=1e-2, beta1=0.9, beta2=0.999, eps=1e-8)], group_of, [0])
    out = {}
    for i in range(2):
        pre()
        logits, loss = e.forward_backward(d.images, d.labels)
        _put(out, **{f"logits{i}": logits, f"loss{i}": loss})
        pre()
        e.optimizer_step(plan)
    return out


def call_bce(e, d, pre):
    out = {}
    for i in range(2):
        pre()
        logits, loss = e.train_step(d.images, d.targets, **STEP)
        _put(out, **{f"logits{i}": logits, f"loss{i}": loss})
    return out


def call_u8(e, d, pre):
    out = {}
    pre()
    logits, loss = e.train_step(d.u8, d.labels, **STEP)
    _put(out, logits=logits, loss=loss)
    return out


def call_u8_resize(e, d, pre):
    out = {}
    e.set_input_resize(True)
    pre()
    logits, loss = e.train_step(d.u8_native, d.labels, **STEP)
    _put(out, logits=logits, loss=loss)
    return out


def call_seams(e, d, pre):
    out = {}
    e.zero_grad()
    pre()
    feat = e.visual_forward(d.images, save=True)
    logits, loss, dfeat = e.head_forward_backward(feat, d.labels)
    e.visual_backward(dfeat)
    _put(out, feat=feat, logits=logits, loss=loss, dfeat=dfeat)
    return out


def call_visual_forward_nosave(e, d, pre):
    out = {}
    pre()
    _put(out, feat=e.visual_forward(d.images, save=False))
    return out


def call_transformer(e, d, pre):
    out = {}
    e.zero_grad()
    pre()
    y = e.transformer_forward(d.x, save=True)
    _put(out, y=y, dx=e.transformer_backward(d.dy))
    return out


def call_blocks(e, d, pre):
    out, lo, hi = {}, 1, e.arch.layers
    e.zero_grad()
    pre()
    y = e.blocks_forward(d.x, lo, hi, save=True)
    _put(out, y=y, dx=e.blocks_backward(d.dy, lo, hi))
    return out


def call_blocks_one_by_one(e, d, pre):
    """The one region that is MEANT to carry state across calls: every block keeps its saved activations in its own slots, so
    that reference-side code can walk resblocks one call per block and differentiate in reverse.  The poison goes before the
    first forward of the walk only; its forward is the launches of transformer_forward."""
    out, L = {}, e.arch.layers
    e.zero_grad()
    pre()
    y = d.x
    for l in range(L):
        y = e.blocks_forward(y, l, l + 1, save=True)
    dx = d.dy
    for l in reversed(range(L)):
        dx = e.blocks_backward(dx, l, l + 1)
    _put(out, y=y, dx=dx)
    assert torch.equal(y, e.transformer_forward(d.x, save=False))
    return out


def call_attention(e, d, pre):
    out, layer = {}, e.arch.layers - 1
    e.zero_grad()
    for form in ("mean", "heads"):
        pre()
        y, w = e.attention_forward(d.x, layer, save=True, weights=form)
        _put(out, **{"y_" + form: y, "weights_" + form: w, "dx_" + form: e.attention_backward(d.dy, layer)})
    return out


def call_dp_halves(e, d, pre):
    """What forward_backward_dp(mode="staged") runs between its exchanges"""
    from pevit_amd import _lib
    out, L = {}, e.arch.layers
    mid = L // 2
    e.zero_grad()
    pre()
    feat = e.visual_forward(d.images, save=True)
    logits, loss, dfeat = e.head_forward_backward(feat, d.labels)
    _lib.check(e.lib.pevit_visual_backward_part(e._ctx, _lib.stream_ptr(), _lib.ptr(dfeat), d.B, L, mid), "upper half")
    _put(out, grads_after_upper_half=e.grads)
    _lib.check(e.lib.pevit_visual_backward_part(e._ctx, _lib.stream_ptr(), None, d.B, mid, 0), "lower half")
    _put(out, feat=feat, logits=logits, loss=loss, dfeat=dfeat)
    return out


def call_predict(e, d, pre):
    out = {}
    pre()
    logits, feat = e.predict(d.images, return_features=True)
    _put(out, logits=logits, feat=feat)
    pre()
    _put(out, logits_u8=e.predict(d.u8))
    return out


def call_encode_image(e, d, pre):
    out = {}
    pre()
    _put(out, feat=e.encode_image(d.images))
    return out


def call_zeroshot(e, d, pre):
    out = {}
    pre()
    probs, logits, feat = e.zeroshot(d.images, d.text, return_logits=True, return_features=True)
    _put(out, probs=probs, logits=logits, feat=feat)
    pre()
    _put(out, probs_alone=e.zeroshot(d.images, d.text))         # the features stay in the workspace here
    return out


def call_probe(e, d, pre):
    out = {}
    for i in range(2):
        pre()
        logits, loss = e.probe_step(d.feats, d.index, d.flabels, **STEP)
        _put(out, **{f"logits{i}": logits, f"loss{i}": loss})
    pre()
    _put(out, predicted=e.probe_predict(d.feats, d.index))
    return out


def call_captured(e, d, pre):
    out = {}
    pre()
    e.train_step(d.images, d.labels, **STEP)                    # capture_train_step asks for one eager step
    pre()
    replay = e.capture_train_step(d.images, d.labels, **STEP)
    for i in range(2):
        pre()
        logits, loss = replay()
        _put(out, **{f"logits{i}": logits, f"loss{i}": loss})
    torch.cuda.synchronize()
    return out


CALLS = {"train3": call_train3, "fb_sgd": call_fb_sgd, "fb_adam": call_fb_adam, "bce": call_bce, "u8": call_u8,
         "u8_resize": call_u8_resize, "seams": call_seams, "visual_forward_nosave": call_visual_forward_nosave,
         "transformer": call_transformer, "blocks": call_blocks, "blocks_one_by_one": call_blocks_one_by_one,
         "attention": call_attention, "dp_halves": call_dp_halves,
         "predict": call_predict, "encode_image": call_encode_image, "zeroshot": call_zeroshot, "probe": call_probe,
         "captured": call_captured}

# (arch, max_batch, odd batch below it)
TOWERS = {"tiny-128": (8, 5), "tiny-256": (5, 3), "tiny-n257": (4, 3)}
CASES = [(a, m, f) for a in TOWERS for f in ("bf16", "f32-verify", "fp8", "fp8-act")
         for m in ("kadaptation", "lora", "adapter", "compacter", "none") if not (f.startswith("fp8") and m in ("adapter", "compacter"))]


def fused_form_is_planned(arch_name, method, weight_format):
    """plan_step (csrc/ctx.hip): an attention-site method, neither f32-verify nor fp8-act, a geometry attn_delta.hip takes"""
    return arch_name == "tiny-128" and method in ("kadaptation", "lora") and weight_format in ("bf16", "fp8")


RUNS = [(a, m, f, b) for a, m, f in CASES for b in ("max", "odd") + (("two-kernel",) if fused_form_is_planned(a, m, f) else ())]


def refused_by_construction(call, method, weight_format):
    return (call == "attention" and weight_format == "fp8-act") or (call == "probe" and method != "none")


@pytest.mark.parametrize("call", list(CALLS))
@pytest.mark.parametrize("arch_name,method,weight_format,batch", RUNS)
def test_every_entry_point_is_self_contained_under_poison(arch_name, method, weight_format, batch, call):
    from pevit_amd import _lib
    max_batch, odd = TOWERS[arch_name]
    arch, p, q = pair(arch_name, method, weight_format, max_batch)
    B = max_batch if batch == "max" else odd
    if batch == "two-kernel":
        hpw = p.lib.pevit_op_attn_delta_hpw
        assert hpw(B, arch.heads, arch.tokens) > 0
        refused = [b for b in range(2, max_batch + 1) if hpw(b, arch.heads, arch.tokens) == 0]
        if refused:                             # a batch the fused form refuses: the two kernels at the default knobs
            B = refused[-1]
        else:                                   # none does (module docstring): the knob, on both engines
            for e in (p, q):
                e.tune("fused_attn_delta", 0)
    d = inputs(arch_name, B)
    fn = CALLS[call]
    if refused_by_construction(call, method, weight_format):
        for e in (p, q):
            before = engine_state(e)
            with pytest.raises(_lib.PevitError):
                fn(e, d, lambda e=e: poison(e))
            assert_flags_clear(e)
            assert differences(engine_state(e), before) == []
        return
    got = fn(p, d, lambda: poison(p))
    want = fn(q, d, lambda: None)
    got.update(engine_state(p)); want.update(engine_state(q))
    assert_flags_clear(p); assert_flags_clear(q)
    assert len(got) > 6 and any(float(v.abs().max()) > 0 for k, v in want.items() if not k.startswith("state."))
    assert differences(want, want) == []        # Q itself is finite
    assert differences(got, want) == []


# ---- 3. one context, the reference's call order ----------------------------------------------------------------------------------
SCRIPT = [("train", 8), ("train", 5), ("predict", 7), ("train", 8), ("encode_image", 3), ("zeroshot", 8), ("train", 2),
          ("probe_step", 4), ("train", 8), ("reset_run", 0), ("train", 6), ("ensure_batch", 12), ("train", 12), ("train", 8)]


def copy_state(dst, src):
    """The walker's parameters, optimizer state, BatchNorm buffers and step count into a control"""
    torch.cuda.synchronize()
    for name in ("params", "grads", "momentum", "running_mean", "running_var"):
        getattr(dst, name).copy_(getattr(src, name))
    dst._steps, dst._optim_kind = src._steps, src._optim_kind


@pytest.mark.parametrize("arch_name,method", [("tiny-128", "kadaptation"), ("tiny-128", "lora"), ("tiny-128", "adapter"),
                                              ("tiny-128", "compacter"), ("tiny-128", "none"), ("tiny-256", "adapter"),
                                              ("tiny-n257", "kadaptation"), ("tiny-n257", "adapter")])
def test_one_context_walks_the_reference_call_order(arch_name, method):
    """train_one with a partial last batch, validate at another batch through the inference layout, the next epoch, the next run
    of the sweep (reset_run; the harness then initialises the trainable tensors again: here to the values the engine was built
    with) and a larger batch (ensure_batch), all on ONE context."""
    from pevit_amd import _lib
    arch, walker = build(arch_name, method, "bf16", 8)
    init = (walker.params.clone(), walker.running_mean.clone(), walker.running_var.clone())
    arena0 = walker.arena.clone()       # (every step rebuilds the adapter panels in the arena: compared as loaded)
    controls = {}

    def control(B):
        if B not in controls:
            controls[B] = build(arch_name, method, "bf16", B)[1]
            assert torch.equal(controls[B].arena, arena0)
        copy_state(controls[B], walker)
        return controls[B]

    def both(B, fn):
        """the same call on the poisoned walker and on the control for its batch, which has just taken the walker's state"""
        c = control(B)
        poison(walker)
        got, want = fn(walker), fn(c)
        got.update(engine_state(walker)); want.update(engine_state(c))
        assert differences(want, want) == [] and differences(got, want) == [], (step, kind, B)
        assert walker._steps == c._steps

    def out(**tensors):
        o = {}
        _put(o, **tensors)
        return o

    trained = 0
    for step, (kind, B) in enumerate(SCRIPT):
        d = inputs(arch_name, B) if B else None
        if kind == "train":
            both(B, lambda e: out(**dict(zip(("logits", "loss"), e.train_step(d.images, d.labels, **STEP)))))
            trained += 1
        elif kind == "predict":
            both(B, lambda e: out(**dict(zip(("logits", "feat"), e.predict(d.images, return_features=True)))))
        elif kind == "encode_image":
            both(B, lambda e: out(feat=e.encode_image(d.images)))
        elif kind == "zeroshot":
            both(B, lambda e: out(probs=e.zeroshot(d.images, d.text)))
        elif kind == "probe_step" and method == "none":
            both(B, lambda e: out(**dict(zip(("logits", "loss"), e.probe_step(d.feats, d.index, d.flabels, **STEP)))))
        elif kind == "probe_step":              # the adapter methods train through train_step: refused on the host, nothing moves
            before = engine_state(walker)
            poison(walker)
            with pytest.raises(_lib.PevitError, match="PEVIT_NONE"):
                walker.probe_step(d.feats, d.index, d.flabels, **STEP)
            assert differences(engine_state(walker), before) == []
        elif kind == "reset_run":
            poison(walker)
            walker.reset_run()
            walker.params.copy_(init[0]); walker.running_mean.copy_(init[1]); walker.running_var.copy_(init[2])
            assert walker._steps == 0
        elif kind == "ensure_batch":
            poison(walker)
            walker.ensure_batch(B)
            assert walker.max_batch == B and walker.workspace.numel() == walker.lib.pevit_workspace_bytes(walker._ctx, B)
        assert_flags_clear(walker)
    assert trained == 8 and float(walker.momentum.abs().max()) > 0


@pytest.mark.parametrize("intruder", ["predict", "probe_step", "encode_image", "transformer_forward", "ensure_batch"])
def test_a_backward_after_another_forward_is_refused(intruder):
    """The saved activations of visual_forward at batch 8 are gone once any other call has laid the workspace out for batch 4 --
    or once ensure_batch has bound another, uninitialised workspace: visual_backward must say so on the host -- no launch,
    gradients and flags as they were."""
    from pevit_amd import _lib
    arch, eng = build("tiny-128", "none" if intruder == "probe_step" else "kadaptation", "bf16", 8)
    d8, d4 = inputs("tiny-128", 8), inputs("tiny-128", 4)
    poison(eng)
    feat = eng.visual_forward(d8.images, save=True)
    _, _, dfeat = eng.head_forward_backward(feat, d8.labels)
    {"predict": lambda: eng.predict(d4.images), "encode_image": lambda: eng.encode_image(d4.images),
     "probe_step": lambda: eng.probe_step(d4.feats, d4.index, d4.flabels, **STEP),
     "transformer_forward": lambda: eng.transformer_forward(d4.x), "ensure_batch": lambda: eng.ensure_batch(12)}[intruder]()
    eng.grads.fill_(3.0)
    torch.cuda.synchronize()
    with pytest.raises(_lib.PevitError, match="saved activations"):
        eng.visual_backward(dfeat)
    torch.cuda.synchronize()
    assert bool((eng.grads == 3.0).all())
    assert_flags_clear(eng)


@pytest.mark.parametrize("pending", [False, True], ids=["after_a_step", "forward_pending"])
def test_the_head_alone_at_a_larger_batch_than_the_last_saving_forward(pending):
    """Host state that decides reads: ``head_forward_backward`` keeps the layout of the last saving forward, so that a pending
    backward finds its activations.  At a LARGER batch than that forward's, the head's slots of that layout are too small and
    overlap each other: the head must lay the workspace out for its own batch -- the bits of the same call on a fresh context --
    and a backward through the smaller forward, whose activations that gives up, must be refused."""
    from pevit_amd import _lib
    arch, eng = build("tiny-128", "kadaptation", "bf16", 8)
    ctl = build("tiny-128", "kadaptation", "bf16", 8)[1]
    d2, d8 = inputs("tiny-128", 2), inputs("tiny-128", 8)
    feats8 = d8.feats[:8].contiguous()
    poison(eng)
    if pending:
        feat2 = eng.visual_forward(d2.images, save=True)
    else:
        eng.train_step(d2.images, d2.labels, **STEP)
        poison(eng)
    copy_state(ctl, eng)
    got = dict(zip(("logits", "loss", "dfeat"), eng.head_forward_backward(feats8, d8.labels)))
    want = dict(zip(("logits", "loss", "dfeat"), ctl.head_forward_backward(feats8, d8.labels)))
    got.update(engine_state(eng)); want.update(engine_state(ctl))
    assert differences(want, want) == [] and differences(got, want) == []
    if pending:
        before = engine_state(eng)
        with pytest.raises(_lib.PevitError, match="saved activations"):
            eng.visual_backward(torch.ones_like(feat2))
        assert differences(engine_state(eng), before) == []
    assert_flags_clear(eng)


def test_the_head_at_a_smaller_batch_keeps_the_pending_forward():
    """... and the other side of it: a forward-only head call on FEWER rows between visual_forward and its backward runs in the
    head slots of the pending forward's layout and changes nothing the backward reads."""
    arch, eng = build("tiny-128", "kadaptation", "bf16", 8)
    ctl = build("tiny-128", "kadaptation", "bf16", 8)[1]
    d8, d4 = inputs("tiny-128", 8), inputs("tiny-128", 4)
    feats4 = d4.feats[:4].contiguous()
    poison(eng)
    outs = []
    for e in (eng, ctl):
        e.zero_grad()
        feat = e.visual_forward(d8.images, save=True)
        if e is eng:
            e.head_forward_backward(feats4, None, bn_training=False)
        logits, loss, dfeat = e.head_forward_backward(feat, d8.labels)
        e.visual_backward(dfeat)
        o = {}
        _put(o, feat=feat, logits=logits, loss=loss, dfeat=dfeat)
        outs.append({**o, **engine_state(e)})
    assert float(outs[1]["state.grads"].abs().max()) > 0
    assert differences(outs[1], outs[1]) == [] and differences(outs[0], outs[1]) == []
    assert_flags_clear(eng)


# ---- 4. the text tower -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight_format", ["bf16", "f32-verify"])
def test_text_tower_is_self_contained_under_poison(weight_format):
    from pevit_amd.text_engine import TextEngine
    from test_text_host import load_text_fixture
    _, _, arch, sd = load_text_fixture("w128_l2_n8")
    g = torch.Generator().manual_seed(23)
    p, q = (TextEngine(arch, max_prompts=6, weight_format=weight_format) for _ in range(2))
    for e in (p, q):
        e.load_state_dict(sd)
    assert torch.equal(p.arena, q.arena)
    for S in (6, 3, 14):                        # max_prompts, fewer, and a set that is split into calls of 6, 6 and 2
        tokens = torch.randint(1, arch.vocab_size, (S, arch.context_length), generator=g)
        poison(p)
        got, want = {"features": p.encode(tokens)}, {"features": q.encode(tokens)}
        torch.cuda.synchronize()
        assert float(want["features"].abs().max()) > 0
        assert differences(want, want) == [] and differences(got, want) == [], S
        assert_flags_clear(p); assert_flags_clear(q)
