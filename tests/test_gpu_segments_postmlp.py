"""Segmented predict for the post-MLP methods (Adapter, Compacter) on the GPU: include/pevit_segments_all.h,
``InferenceEngine(..., "adapter" | "compacter", slots=2..8).predict_segments``.

1. ``adapter_fwd_seg_kernel`` (csrc/adapter_fused.hip) through ``pevit_op_adapter_fwd_seg`` against ``pevit_op_adapter_fwd_ex`` called
   once per segment on that segment's row slices with that segment's weights: ``x_out`` bit for bit, on small tables and row by
   row at serving size (25 600 rows).  The segmented entry and its launcher take no z / act / apre / mean_a / rstd_a pointer at
   all -- the launcher hands the kernel NULL for the five -- so "nothing that only a backward reads is stored" holds by
   construction; what the test can and does check is that ``x_out`` is written on the segments' rows only (NaN pre-fill, sentinel
   guard rows) and that the operands come back untouched.
2. One segment in slot 2 of a four-slot context is ``use(name); predict(images)`` on a plain context: bit for bit, on the unfused
   route (tiny-128, or "adapter_fused" tuned 0) and on the fused one (tiny-256).
3. Segments do not leak: every segment of a mixed call (a, b, a) equals the same segment of the all-a / all-b call: bit for bit.
4. Segments are their own batches: against ``use(name); predict(images[segment])`` under the gate of tests/test_gpu_segments.py
   (``FLOOR_C`` x the plan floor measured on method "none"); the floor must be 0 on both tiny arches, where the gate is bit equality.
5. Two Compacter adapters with different frozen rules in two slots while a third is selected: each segment has its own bits and the
   selected adapter's next ``predict`` is unchanged (loading a slot does not pass through the arena's rule).
6. Interleaving with the single-adapter calls, self-containment under workspace poison, and no panel-building launch once the slots
   are loaded (the f32 sources of the panels, Compacter's rule included, are overwritten and nothing changes).
7. uint8 requests at tower size.  8. Every refusal comes before any launch.  9. ``predict_mixed``: rows are independent."""
import ctypes as C
import functools

import pytest
import torch

from conftest import FLOOR_C, max_rel

from test_gpu_adapter_fused import guarded, intact
from test_gpu_predict import P, S, ok, rnd
from test_gpu_segments import as_dicts, engine, plan_floor, requests_of, two_adapters
from test_gpu_serving import ARCH_BATCH, images_of, same_bits
from test_gpu_workspace import assert_flags_clear, differences, poison

pytestmark = pytest.mark.gpu

ARCHES = ("tiny-128", "tiny-256")           # E = 128: the unfused route whatever the knob; E = 256: the fused route (NV = 1)
METHODS = ("adapter", "compacter")
SEGMENTATION = {"tiny-128": (3, 1, 4), "tiny-256": (2, 1, 2)}
BF = torch.bfloat16


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from pevit_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module", autouse=True)
def _cleanup():
    yield
    mixed_runs.cache_clear()


# ---- 1. the kernel ------------------------------------------------------------------------------------------------------------------
def weights(E, seed):
    return dict(gamma=1 + rnd(E, seed=seed, scale=0.2), beta=rnd(E, seed=seed + 1, scale=0.2),
                wd=rnd(64, E, seed=seed + 2, scale=E ** -0.5, dtype=BF), b_down=rnd(64, seed=seed + 3, scale=0.1),
                wu=rnd(E, 64, seed=seed + 4, scale=0.125, dtype=BF), b_up=rnd(E, seed=seed + 5, scale=0.1))


def fwd_ex(lib, act, E, hraw, bpr, x_mid, w):
    """the unsegmented kernel on these rows alone: x_out"""
    from pevit_amd._lib import PevitAdapterFwdArgs
    T = hraw.shape[0]
    buf = dict(z=torch.empty((T, E), dtype=BF, device="cuda"), mean_a=torch.empty(T, device="cuda"), rstd_a=torch.empty(T, device="cuda"),
               act=torch.empty((T, 64), dtype=BF, device="cuda"), apre=torch.empty((T, 64), dtype=BF, device="cuda"),
               x_out=torch.full((T, E), float("nan"), device="cuda"))
    a = PevitAdapterFwdArgs()
    a.act_kind, a.T, a.E = act, T, E
    a.hraw, a.bpr, a.x_mid = hraw.data_ptr(), bpr.data_ptr(), x_mid.data_ptr()
    for k, t in list(w.items()) + list(buf.items()):
        assert t.is_contiguous()
        setattr(a, k, t.data_ptr())
    ok(lib, lib.pevit_op_adapter_fwd_ex(S(), C.byref(a)))
    torch.cuda.synchronize()
    return buf["x_out"]


def seg_args(act, E, hraw, bpr, x_mid, x_out, table):
    """table = [(first row, end row, weights)]; returns the argument struct and what must stay alive behind it"""
    from pevit_amd._lib import PevitAdapterFwdSegArgs, PevitAdapterSeg
    segs = (PevitAdapterSeg * max(len(table), 1))()
    for g, (first, end, w) in zip(segs, table):
        g.first, g.end = first, end
        for k, t in w.items():
            setattr(g, k, t.data_ptr())
    a = PevitAdapterFwdSegArgs()
    a.hraw, a.bpr, a.x_mid, a.x_out, a.segs = hraw.data_ptr(), bpr.data_ptr(), x_mid.data_ptr(), x_out.data_ptr(), segs
    a.act_kind, a.E, a.nseg = act, E, len(table)
    return a, segs


@pytest.mark.parametrize("N,counts", [(10, (3, 1, 4)), (10, (1,) * 8), (10, (8,)), (16, (2, 2))])
@pytest.mark.parametrize("E", [256, 768, 1024])
@pytest.mark.parametrize("act", [0, 1])
def test_the_kernel_by_segments_is_the_kernel_per_segment(lib, act, E, N, counts):
    """N = 10, (3, 1, 4): rows 30 | 10 | 40 -- a segment end inside a tile, a segment smaller than a tile, one of a full tile plus
    8 rows; eight segments of 10 rows; one segment (also the unsegmented kernel on the whole); N = 16, (2, 2): segments of exactly
    32 rows.  Every segment has its own weights, assigned in reverse order."""
    T, nseg = sum(counts) * N, len(counts)
    hraw, bpr, x_mid = rnd(T, E, seed=E + T, scale=2.0) + 0.5, rnd(E, seed=E + T + 1, scale=0.5), rnd(T, E, seed=E + T + 2)
    sets = [weights(E, seed=1000 + 10 * i) for i in range(nseg)]
    table, first = [], 0
    for i, c in enumerate(counts):
        table.append((first, first + c * N, sets[nseg - 1 - i]))
        first += c * N
    x_out = guarded(T, E, torch.float32)
    keep = [t.clone() for t in (hraw, bpr, x_mid)]
    a, segs = seg_args(act, E, hraw, bpr, x_mid, x_out, table)
    ok(lib, lib.pevit_op_adapter_fwd_seg(S(), C.byref(a)))
    torch.cuda.synchronize()
    assert intact(x_out, T), "a row behind the last segment was written"
    assert bool(torch.isfinite(x_out[:T]).all()), "a row of a segment was left unwritten"
    for t, k in zip((hraw, bpr, x_mid), keep):
        assert torch.equal(t, k)
    for lo, hi, w in table:
        want = fwd_ex(lib, act, E, hraw[lo:hi], bpr, x_mid[lo:hi], w)
        assert torch.equal(x_out[lo:hi], want), (lo, hi, float((x_out[lo:hi] - want).abs().max()))
    if nseg == 1:
        assert torch.equal(x_out[:T], fwd_ex(lib, act, E, hraw, bpr, x_mid, table[0][2]))
    elif nseg == 3:       # the weights matter: the first segment under the last one's weights differs
        assert not torch.equal(x_out[:table[0][1]], fwd_ex(lib, act, E, hraw[:table[0][1]], bpr, x_mid[:table[0][1]], table[2][2]))


@pytest.mark.parametrize("E", [768, 1024])
@pytest.mark.parametrize("act", [0, 1])
def test_the_kernel_at_serving_size_row_by_row(lib, act, E):
    """8 segments of 64 images of 50 tokens: 25 600 rows.  The small cases above cannot see a kernel that rounds one row in a few
    thousand differently: a first form of the segmented kernel, whose LayerNorm arithmetic the compiler had fused differently at
    NV = 3, passed them all and differed from adapter_fwd_kernel in about one row in 2000 of a ViT-B/32 walk."""
    N, counts = 50, (64,) * 8
    T, nseg = sum(counts) * N, len(counts)
    hraw, bpr, x_mid = rnd(T, E, seed=7, scale=2.0) + 0.5, rnd(E, seed=8, scale=0.5), rnd(T, E, seed=9)
    sets = [weights(E, seed=2000 + 10 * i) for i in range(nseg)]
    table = [(i * 64 * N, (i + 1) * 64 * N, sets[nseg - 1 - i]) for i in range(nseg)]
    x_out = guarded(T, E, torch.float32)
    a, segs = seg_args(act, E, hraw, bpr, x_mid, x_out, table)
    ok(lib, lib.pevit_op_adapter_fwd_seg(S(), C.byref(a)))
    torch.cuda.synchronize()
    assert intact(x_out, T)
    bad = 0
    for lo, hi, w in table:
        want = fwd_ex(lib, act, E, hraw[lo:hi], bpr, x_mid[lo:hi], w)
        bad += int((x_out[lo:hi] != want).any(1).sum())
    assert bad == 0, f"{bad} of {T} rows differ from adapter_fwd_kernel"


def test_a_gap_between_segments_is_not_written(lib):
    """the launcher takes any non-empty row ranges: rows between two segments keep their bits"""
    E, T = 256, 100
    hraw, bpr, x_mid = rnd(T, E, seed=1, scale=2.0), rnd(E, seed=2, scale=0.5), rnd(T, E, seed=3)
    w = weights(E, seed=50)
    x_out = guarded(T, E, torch.float32)
    a, segs = seg_args(0, E, hraw, bpr, x_mid, x_out, [(0, 33, w), (70, 100, w)])
    ok(lib, lib.pevit_op_adapter_fwd_seg(S(), C.byref(a)))
    torch.cuda.synchronize()
    assert bool(torch.isnan(x_out[33:70]).all()) and bool(torch.isfinite(x_out[:33]).all()) and bool(torch.isfinite(x_out[70:100]).all())
    assert intact(x_out, T)


def test_the_kernel_entry_refuses_bad_tables(lib):
    E, T = 256, 40
    hraw, bpr, x_mid = rnd(T, E, seed=1), rnd(E, seed=2), rnd(T, E, seed=3)
    w = weights(E, seed=60)
    x_out = torch.zeros((T, E), device="cuda")

    def call(table, E_=E, nseg=None):
        a, segs = seg_args(0, E_, hraw, bpr, x_mid, x_out, table)
        if nseg is not None:
            a.nseg = nseg
        return lib.pevit_op_adapter_fwd_seg(S(), C.byref(a)), lib.pevit_last_error()
    for kw, word in ((dict(table=[(i, i + 1, w) for i in range(17)]), b"17 segments outside [1,16]"),
                     (dict(table=[], nseg=0), b"0 segments outside"),
                     (dict(table=[(0, 10, w), (10, 10, w)]), b"empty"),
                     (dict(table=[(0, 10, w), (20, 15, w)]), b"empty"),
                     (dict(table=[(0, 40, w)], E_=128), b"unsupported width"),
                     (dict(table=[(0, 40, w)], E_=1280), b"unsupported width")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw.keys(), msg)
    assert lib.pevit_op_adapter_fwd_seg(S(), None) != 0
    torch.cuda.synchronize()
    assert not bool(x_out.any())                                   # nothing was launched


# ---- 2. one segment is predict ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("arch_name", ARCHES)
def test_one_segment_is_predict(arch_name, method, fused):
    arch, ckpts = two_adapters(arch_name, method)
    multi, plain = engine(arch_name, method, ckpts, slots=4), engine(arch_name, method, {"a": ckpts["a"]})
    for e in (multi, plain):
        assert e.tune("adapter_fused", fused) == 0
    assert multi.workspace_bytes == plain.workspace_bytes and multi.arena_bytes > plain.arena_bytes
    multi._load_slot(2, "a")                       # slot 2, with slots 0, 1 and 3 empty
    multi._slot_names[2] = "a"
    plain.use("a")
    big, odd = ARCH_BATCH[arch_name]
    for B in (big, odd, 1):
        img = images_of(arch, B, seed=20 + B)
        want = dict(zip(("logits", "features"), plain.predict(img, return_features=True)))
        got = as_dicts(multi.predict_segments([("a", img)], return_features=True))[0]
        assert got["logits"].shape == (B, 10) and float(got["logits"].abs().max()) > 0
        same_bits(got, want)
        assert_flags_clear(multi)
    assert multi._slot_names == [None, None, "a", None]
    # the single-adapter calls on the slot context are the plain context's, bit for bit
    multi.use("a")
    img = images_of(arch, odd, seed=33)
    same_bits(dict(zip(("logits", "features"), multi.predict(img, return_features=True))),
              dict(zip(("logits", "features"), plain.predict(img, return_features=True))))
    same_bits({"features": multi.encode_image(img)}, {"features": plain.encode_image(img)})
    assert_flags_clear(multi)


# ---- 3. and 4. ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_runs(arch_name, method):
    arch, ckpts = two_adapters(arch_name, method)
    counts = SEGMENTATION[arch_name]
    names = ("a", "b", "a")
    img = images_of(arch, sum(counts), seed=77)
    multi = engine(arch_name, method, ckpts, slots=2)
    runs = {"mixed": as_dicts(multi.predict_segments(requests_of(img, counts, names), return_features=True))}
    for n in ("a", "b"):
        runs[n] = as_dicts(multi.predict_segments(requests_of(img, counts, (n,) * len(counts)), return_features=True))
    assert_flags_clear(multi)
    plain = engine(arch_name, method, ckpts)
    alone, lo = [], 0
    for c, n in zip(counts, names):
        plain.use(n)
        alone.append(dict(zip(("logits", "features"), (x.clone() for x in plain.predict(img[lo:lo + c], return_features=True)))))
        lo += c
    torch.cuda.synchronize()
    return counts, names, img, runs, alone


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("arch_name", ARCHES)
def test_segments_do_not_leak(arch_name, method):
    counts, names, img, runs, alone = mixed_runs(arch_name, method)
    for i, n in enumerate(names):
        same_bits(runs["mixed"][i], runs[n][i])
    assert not torch.equal(runs["a"][0]["features"], runs["b"][0]["features"])
    assert runs["a"][0]["logits"].shape[1] == 10 and runs["b"][0]["logits"].shape[1] == 7


@functools.lru_cache(maxsize=None)
def floor_of(arch_name):
    counts = SEGMENTATION[arch_name]
    from pevit_amd.synth import ARCHS
    return plan_floor(arch_name, counts, images_of(ARCHS[arch_name], sum(counts), seed=77))


def test_the_plan_floor_is_zero_on_both_tiny_arches():
    """the gate of the next test is FLOOR_C x floor: it is bit equality only where the floor is 0"""
    floors = {a: floor_of(a) for a in ARCHES}
    print("plan floors:", floors)
    assert all(f == 0.0 for f in floors.values()), floors


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("arch_name", ARCHES)
def test_segments_are_their_own_batches(arch_name, method):
    counts, names, img, runs, alone = mixed_runs(arch_name, method)
    floor = floor_of(arch_name)
    gate = FLOOR_C * floor
    dist = [max(max_rel(runs["mixed"][i][k], alone[i][k]) for k in ("logits", "features")) for i in range(len(counts))]
    print(f"{arch_name} {method}: segments {counts} slots {names}: plan floor {floor:.3e}, gate {gate:.3e}, distances "
          + ", ".join(f"{d:.3e}" for d in dist))
    for i, d in enumerate(dist):
        assert d <= gate, (i, d, gate)
        if gate == 0.0:
            same_bits(runs["mixed"][i], alone[i])


# ---- 5. Compacter rules -------------------------------------------------------------------------------------------------------------
def with_rule(ckpt, seed):
    rule = torch.rand((4, 4, 4), generator=torch.Generator().manual_seed(seed)) * 2 - 1
    t = dict(ckpt["tensors"])
    assert t["visual.transformer.phm_rule"].shape == rule.shape
    t["visual.transformer.phm_rule"] = rule
    return dict(ckpt, meta=dict(ckpt["meta"]), tensors=t)


@pytest.mark.parametrize("arch_name", ARCHES)
def test_compacter_slots_keep_their_own_rules_and_leave_the_selected_one_alone(arch_name):
    arch, ckpts = two_adapters(arch_name, "compacter")
    ckpts = {"a": ckpts["a"], "b": with_rule(ckpts["b"], 21), "c": with_rule(ckpts["a"], 22), "a_rule_c": with_rule(ckpts["a"], 22)}
    multi = engine(arch_name, "compacter", ckpts, slots=2)
    counts = SEGMENTATION[arch_name][:2]
    img = images_of(arch, sum(counts), seed=41)
    multi.use("c")
    before = dict(zip(("logits", "features"), (x.clone() for x in multi.predict(img, return_features=True))))
    mixed = as_dicts(multi.predict_segments(requests_of(img, counts, ("a", "b")), return_features=True))
    assert sorted(multi._slot_names) == ["a", "b"]
    after = dict(zip(("logits", "features"), multi.predict(img, return_features=True)))      # c is still selected
    same_bits(after, before)
    for i, n in enumerate(("a", "b")):
        whole = as_dicts(multi.predict_segments(requests_of(img, counts, (n, n)), return_features=True))
        same_bits(mixed[i], whole[i])
    # each against the plain context, where `use` carries the rule through the arena: the same row count, and (test 4) a zero floor
    plain = engine(arch_name, "compacter", ckpts)
    lo = 0
    for i, (c, n) in enumerate(zip(counts, ("a", "b"))):
        plain.use(n)
        same_bits(mixed[i], dict(zip(("logits", "features"), plain.predict(img[lo:lo + c], return_features=True))))
        lo += c
    # ... and the rule matters: a's parameters under c's rule give other bits
    plain.use("a_rule_c")
    assert not torch.equal(plain.predict(img[:counts[0]], return_features=True)[1], mixed[0]["features"])
    assert_flags_clear(multi)


# ---- 6. interleaving, poison, no panel-building launch ------------------------------------------------------------------------------
def overwrite_panel_sources(e, name, method, arch):
    """NaN over what the panels were built from; the LayerNorm affine, b_down, b_up and the head are read in place and stay"""
    E, L = arch.width, arch.layers
    p = e._adapters[name]["params"]
    if method == "adapter":
        stride = 2 * E + 64 * E + 64 + 64 * E + E
        for l in range(L):
            p[stride * l + 2 * E:stride * l + 2 * E + 64 * E].fill_(float("nan"))                            # adapter_down weight
            p[stride * l + 2 * E + 64 * E + 64:stride * l + 2 * E + 64 * E + 64 + 64 * E].fill_(float("nan"))  # adapter_up weight
    else:
        stride = 2 * E + E + 64 + 64 + 64 + E + E
        for l in range(L):
            p[stride * l + 2 * E:stride * l + 2 * E + E + 64].fill_(float("nan"))                            # down W_left, W_right
            p[stride * l + 2 * E + E + 128:stride * l + 2 * E + E + 128 + 64 + E].fill_(float("nan"))        # up W_left, W_right
        e._adapters[name]["phm_rule"].fill_(float("nan"))
    assert stride * L == e.n_tower


@pytest.mark.parametrize("arch_name,method", [("tiny-128", "adapter"), ("tiny-128", "compacter"), ("tiny-256", "adapter"), ("tiny-256", "compacter")])
def test_interleaved_with_single_adapter_calls_and_self_contained_under_poison(arch_name, method):
    arch, ckpts = two_adapters(arch_name, method)
    counts = SEGMENTATION[arch_name]
    names = ("a", "b", "a")
    PP, Q, plain = engine(arch_name, method, ckpts, slots=2), engine(arch_name, method, ckpts, slots=2), engine(arch_name, method, ckpts)
    img = images_of(arch, sum(counts), seed=61)
    reqs = requests_of(img, counts, names)
    first = as_dicts(Q.predict_segments(reqs, return_features=True))
    assert_flags_clear(Q)
    for e in (Q, plain):
        e.use("b")
    between = dict(zip(("logits", "features"), Q.predict(img, return_features=True)))
    assert_flags_clear(Q)
    same_bits(between, dict(zip(("logits", "features"), plain.predict(img, return_features=True))))
    again = as_dicts(Q.predict_segments(reqs, return_features=True))
    for a, b in zip(first, again):
        same_bits(b, a)
    # poison: PP is filled with NaN bytes before every call, Q keeps the leftovers of whatever ran before
    big, odd = ARCH_BATCH[arch_name]
    for n_img in (sum(counts), odd, 1):
        im = images_of(arch, n_img, seed=60 + n_img)
        cs = counts if n_img == sum(counts) else ((n_img - 1, 1) if n_img > 1 else (1,))
        rq = requests_of(im, cs, ("b", "a", "b")[:len(cs)])
        poison(PP)
        got, want = PP.predict_segments(rq, return_features=True), Q.predict_segments(rq, return_features=True)
        for g, w in zip(as_dicts(got), as_dicts(want)):
            bad = differences(g, w)
            assert not bad, (n_img, bad)
        assert_flags_clear(PP)
    # the slots are loaded: overwrite the f32 sources of the panels
    assert sorted(PP._slot_names) == ["a", "b"]
    want = as_dicts(PP.predict_segments(reqs, return_features=True))
    n_loads = []
    PP._load_slot = lambda slot, name: n_loads.append(name)
    for n in ("a", "b"):
        overwrite_panel_sources(PP, n, method, arch)
    poison(PP)
    got = as_dicts(PP.predict_segments(reqs, return_features=True))
    for g, w in zip(got, want):
        same_bits(g, w)
    assert not n_loads
    assert_flags_clear(PP)


# ---- 7. uint8 requests ----------------------------------------------------------------------------------------------------------------
def test_uint8_requests_at_tower_size():
    from test_gpu_serving import MEAN, STD
    arch_name, method = "tiny-256", "adapter"
    arch, ckpts = two_adapters(arch_name, method)
    multi, plain = engine(arch_name, method, ckpts, slots=2), engine(arch_name, method, ckpts)
    counts, names = SEGMENTATION[arch_name], ("a", "b", "a")
    n, R = sum(counts), arch.resolution
    exact = torch.randint(0, 256, (n, 3, R, R), generator=torch.Generator().manual_seed(8), dtype=torch.uint8).cuda()
    with pytest.raises(Exception, match="float32"):
        multi.predict_segments(requests_of(exact, counts, names))          # uint8 before set_input_normalization
    for e in (multi, plain):
        e.set_input_normalization(MEAN, STD)
    got = as_dicts(multi.predict_segments(requests_of(exact, counts, names), return_features=True))      # pevit_predict_segments_u8
    lo = 0
    for i, (c, nm) in enumerate(zip(counts, names)):
        plain.use(nm)
        same_bits(got[i], dict(zip(("logits", "features"), plain.predict(exact[lo:lo + c], return_features=True))))
        lo += c
    assert_flags_clear(multi)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_every_refusal_comes_before_any_launch(lib, method):
    from pevit_amd import _lib
    arch, ckpts = two_adapters("tiny-128", method)
    multi, plain = engine("tiny-128", method, ckpts, slots=4), engine("tiny-128", method, ckpts)
    img = images_of(arch, 8, seed=5)
    good = multi.predict_segments([("a", img[:3]), ("b", img[3:])])            # slots 0 and 1 are loaded from here on
    torch.cuda.synchronize()
    poison(multi)
    before = multi.workspace.clone()
    a = multi._adapters["a"]
    out = torch.zeros((8, 10), device="cuda")

    def call(ctx, table, B=8, nseg=None):
        segs = (_lib.PevitSegment * max(len(table), 1))()
        for g, (first, count, slot) in zip(segs, table):
            g.first, g.count, g.slot = first, count, slot
            g.running_mean, g.running_var, g.logits = a["running_mean"].data_ptr(), a["running_var"].data_ptr(), out.data_ptr()
        big = torch.zeros((max(B, 1), 3, arch.resolution, arch.resolution), device="cuda")
        rc = lib.pevit_predict_segments(ctx, _lib.stream_ptr(), _lib.ptr(big), B, len(table) if nseg is None else nseg, segs)
        return rc, lib.pevit_last_error()
    for table, kw, word in (([(0, 3, 0), (4, 4, 1)], {}, b"must tile"),                      # a gap
                            ([(0, 5, 0), (3, 5, 1)], {}, b"must tile"),                      # an overlap
                            ([(0, 3, 0), (3, 4, 1)], {}, b"cover 7 of 8"),
                            ([(0, 3, 0), (3, 6, 1)], {}, b"must tile"),                      # past the end
                            ([(0, 0, 0), (0, 8, 1)], {}, b"must tile"),                      # an empty segment
                            ([(0, 3, 0), (3, 5, 2)], {}, b"not loaded"),
                            ([(0, 3, 0), (3, 5, 4)], {}, b"outside [0,4)"),
                            ([(i, 1, 0) for i in range(17)], dict(B=8), b"17 segments outside [1,16]"),
                            ([], dict(nseg=0), b"0 segments outside"),
                            ([(0, 9, 0)], dict(B=9), b"batch 9 outside [1,8]")):
        rc, msg = call(multi._ctx, table, **kw)
        assert rc != 0 and word in msg, (table, msg)
    rc, msg = call(plain._ctx, [(0, 8, 0)])
    assert rc != 0 and b"no adapter slots" in msg
    # the loaders: a rule on an Adapter context, none on a Compacter one -- before anything is built
    fake = a["running_mean"]
    if method == "adapter":
        rc = lib.pevit_load_adapter_slot_rule(multi._ctx, _lib.stream_ptr(), 0, _lib.ptr(a["params"]), 10, _lib.ptr(fake))
        assert rc != 0 and b"only Compacter" in lib.pevit_last_error()
    else:
        rc = lib.pevit_load_adapter_slot(multi._ctx, _lib.stream_ptr(), 0, _lib.ptr(a["params"]), 10)
        assert rc != 0 and b"pevit_load_adapter_slot_rule" in lib.pevit_last_error()
    with pytest.raises(_lib.PevitError, match="exceeds max_batch"):
        multi.predict_segments([("a", images_of(arch, 9, seed=6))])
    with pytest.raises(_lib.PevitError, match="slots"):
        plain.predict_segments([("a", img)])
    torch.cuda.synchronize()
    assert torch.equal(multi.workspace, before) and not bool(out.any())        # nothing was launched
    assert_flags_clear(multi)
    again = multi.predict_segments([("a", img[:3]), ("b", img[3:])])           # ... and the refused loads left the slots as they were
    for g, w in zip(again, good):
        same_bits({"logits": g}, {"logits": w})
    # dropping a resident adapter empties its slot; so does load_backbone (pevit_load_block empties every slot)
    multi.drop("b")
    assert multi._slot_names[:2] == ["a", None]
    from test_gpu_serving import backbone
    multi.load_backbone(backbone("tiny-128"))
    assert multi._slot_names == [None] * 4
    rc, msg = call(multi._ctx, [(0, 8, 0)])
    assert rc != 0 and b"not loaded" in msg
    plain.use("a")
    same_bits({"logits": multi.predict_segments([("a", img)])[0]}, {"logits": plain.predict(img)})


# ---- 9. predict_mixed -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch_name,method", [("tiny-128", "compacter"), ("tiny-256", "adapter")])
def test_predict_mixed_is_predict_per_name_and_rows_are_independent(arch_name, method):
    arch, ckpts = two_adapters(arch_name, method)
    multi, plain = engine(arch_name, method, ckpts, slots=2), engine(arch_name, method, ckpts)
    n = ARCH_BATCH[arch_name][0]
    img = images_of(arch, n, seed=88)
    names = (["b", "a", "b", "b", "a", "a", "a", "b"] * 2)[:n]
    full = multi.predict_mixed(img, names)
    assert full.shape == (n, 10)
    for nm, width in (("a", 10), ("b", 7)):
        rows = [i for i, x in enumerate(names) if x == nm]
        plain.use(nm)
        want = plain.predict(img[rows].contiguous())
        same_bits({"logits": full[rows][:, :width].contiguous()}, {"logits": want})
        assert bool((full[rows][:, width:] == float("-inf")).all())
    # permuting the rows of one name permutes its logits, bit for bit: a row's answer depends on no other row
    rows_a = [i for i, x in enumerate(names) if x == "a"]
    perm = list(range(n))
    for src, dst in zip(rows_a, rows_a[1:] + rows_a[:1]):
        perm[dst] = src
    moved = multi.predict_mixed(img[perm].contiguous(), names)
    assert torch.equal(moved, full[perm])                      # (-inf behind a row's class count included)
    assert bool(torch.isfinite(moved[rows_a]).all())
    assert len(rows_a) > 1 and not torch.equal(full[rows_a[0]], full[rows_a[1]])
