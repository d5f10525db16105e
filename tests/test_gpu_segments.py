"""Segmented predict on the GPU: requests for several resident adapters in one engine call (include/pevit_segments.h,
``InferenceEngine.predict_segments``).

1. The two segmented kernels against the unsegmented ones called once per segment on that segment's slices: bit for bit.
2. One segment in slot 2 of a four-slot context is ``use(name); predict(images)`` on a plain context: bit for bit.
3. Segments do not leak: every segment of a mixed call (a, b, a) equals the same segment of the all-a / all-b call: bit for bit.
4. Segments are their own batches: every segment of the mixed call against ``use(name); predict(images[segment])``.  The GEMMs
   behind QKV may be planned differently at another row count, so this gate is measured: ``floor`` = the largest relative difference,
   on method "none" with the same tower and images, between ``predict(images)[segment]`` and ``predict(images[segment])`` -- paths
   this work leaves alone and that are row-wise by definition, so they differ by the plan alone; gate = ``FLOOR_C`` x floor, i.e. bit
   equality wherever the floor is 0.  Measured on an MI355X (profiles/serving_segments.md): the floor is 0 on all three arches and
   every segment is bit-equal.
5. Interleaving with the single-adapter calls, self-containment under workspace poison, no panel-building launch once the slots
   are loaded (the f32 sources of the panels are overwritten after the load and nothing changes).
6. Every refusal comes before any launch.

Arches and batches are those of tests/test_gpu_serving.py: tiny-128 (H = 2, N = 10: the fused form, where a run of six heads is
three images and must not cross a segment), tiny-256 (H = 4, N = 17: the two-kernel form), tiny-n257 (N = 257: the N > 64 branch)."""
import ctypes as C
import functools

import pytest
import torch

from conftest import FLOOR_C, max_rel

from test_gpu_predict import P, S, ok, rnd
from test_gpu_serving import ARCH_BATCH, backbone, images_of, same_bits, trained
from test_gpu_workspace import assert_flags_clear, differences, poison

pytestmark = pytest.mark.gpu

SEGMENTATION = {"tiny-128": (3, 1, 4), "tiny-256": (2, 3), "tiny-n257": (1, 3)}


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


# ---- 1. the kernels ---------------------------------------------------------------------------------------------------------------
def site_case(B, H, N, counts, seed):
    """q, k, v in the head layout, t at pitch 64 * slots with one slot per segment (in reverse order, so that no segment finds its
    columns where its position would put them), one Q panel and one bias per segment (the first segment of several: no bias)."""
    from pevit_amd import _lib
    E, nseg = H * 64, len(counts)
    assert sum(counts) == B
    q = rnd(B * H, N, 64, seed=seed + 1, scale=0.35, dtype=torch.bfloat16)
    k = rnd(B * H, N, 64, seed=seed + 2, dtype=torch.bfloat16)
    v = rnd(B * H, N, 64, seed=seed + 3, dtype=torch.bfloat16)
    t = rnd(B * N, 64 * nseg, seed=seed + 4)
    q16 = [rnd(E, 64, seed=seed + 10 + i, scale=0.3).bfloat16() for i in range(nseg)]
    bias = [None if (i == 0 and nseg > 1) else rnd(E, seed=seed + 40 + i, scale=0.2) for i in range(nseg)]
    segs = (_lib.PevitOpSegment * nseg)()
    first, parts = 0, []
    for i, c in enumerate(counts):
        tcol = 64 * (nseg - 1 - i)
        segs[i].first, segs[i].count, segs[i].tcol = first, c, tcol
        segs[i].q16, segs[i].bias = q16[i].data_ptr(), None if bias[i] is None else bias[i].data_ptr()
        parts.append((first, c, t[first * N:(first + c) * N, tcol:tcol + 64].contiguous(), q16[i], bias[i]))
        first += c
    return E, q, k, v, t, segs, parts, (q16, bias)


@pytest.mark.parametrize("B,H,N,counts", [(8, 2, 10, (3, 1, 4)), (8, 2, 10, (5, 3)), (8, 2, 10, (1,) * 8), (3, 12, 50, (1, 2))])
def test_fused_kernel_by_segments_is_the_fused_kernel_per_segment(lib, B, H, N, counts):
    """H = 2, N = 10: a run of six heads is three images -- the runs of (3, 1, 4) end inside, at and behind segment ends, and eight
    segments of one image are eight partial runs.  H = 12, N = 50: the compile-time instance."""
    E, q, k, v, t, segs, parts, keep = site_case(B, H, N, counts, seed=100)
    assert lib.pevit_op_attn_delta_hpw(B, H, N) == 6
    out = torch.full((B * N, E), float("nan"), dtype=torch.bfloat16, device="cuda")
    q0, v0 = q.clone(), v.clone()
    ok(lib, lib.pevit_op_attn_fwd_delta_seg(S(), P(q), P(k), P(v), P(t), t.shape[1], 160.0, P(out), E, B, H, N, len(counts), segs))
    torch.cuda.synchronize()
    assert torch.equal(q, q0) and torch.equal(v, v0)               # the inference form only reads them
    assert bool(torch.isfinite(out.float()).all()) and float(out.float().abs().max()) > 0
    for first, c, ts, q16, bias in parts:
        qs, ks, vs = (x[first * H:(first + c) * H].contiguous() for x in (q, k, v))
        want = torch.zeros((c * N, E), dtype=torch.bfloat16, device="cuda")
        ok(lib, lib.pevit_op_attn_fwd_delta(S(), P(qs), P(ks), P(vs), P(ts), P(q16), P(bias), 160.0, P(want), E, None, c, H, N))
        torch.cuda.synchronize()
        assert torch.equal(out[first * N:(first + c) * N], want), (first, c)


@pytest.mark.parametrize("B,H,N,counts", [(5, 4, 17, (2, 3)), (5, 4, 17, (1, 4)), (4, 2, 257, (1, 3)), (8, 2, 10, (3, 1, 4))])
def test_delta_add_by_segments_is_delta_add_per_segment(lib, B, H, N, counts):
    """The two-kernel form: the segmented delta-add in front of the unchanged attention kernel."""
    E, q, k, v, t, segs, parts, keep = site_case(B, H, N, counts, seed=200)
    q1, v1 = q.clone(), v.clone()
    ok(lib, lib.pevit_op_delta_add_seg(S(), P(q1), P(v1), P(t), t.shape[1], 160.0, B, H, N, len(counts), segs))
    out = torch.full((B * N, E), float("nan"), dtype=torch.bfloat16, device="cuda")
    ok(lib, lib.pevit_op_attn_fwd(S(), P(q1), P(k), P(v1), P(out), E, None, B, H, N))
    torch.cuda.synchronize()
    assert not torch.equal(q1, q) and not torch.equal(v1, v)
    for first, c, ts, q16, bias in parts:
        qs, ks, vs = (x[first * H:(first + c) * H].clone() for x in (q, k, v))
        ok(lib, lib.pevit_op_delta_add(S(), P(qs), P(vs), P(ts), P(q16), P(bias), 160.0, c, N, E))
        want = torch.zeros((c * N, E), dtype=torch.bfloat16, device="cuda")
        ok(lib, lib.pevit_op_attn_fwd(S(), P(qs), P(ks), P(vs), P(want), E, None, c, H, N))
        torch.cuda.synchronize()
        assert torch.equal(q1[first * H:(first + c) * H], qs) and torch.equal(v1[first * H:(first + c) * H], vs), (first, c)
        assert torch.equal(out[first * N:(first + c) * N], want), (first, c)


def test_the_kernel_entries_refuse_bad_tables(lib):
    E, q, k, v, t, segs, parts, keep = site_case(8, 2, 10, (3, 1, 4), seed=300)
    out = torch.zeros((80, E), dtype=torch.bfloat16, device="cuda")

    def both(nseg=3, pitch=192, B=8):
        a = lib.pevit_op_attn_fwd_delta_seg(S(), P(q), P(k), P(v), P(t), pitch, 160.0, P(out), E, B, 2, 10, nseg, segs)
        msg = lib.pevit_last_error()
        b = lib.pevit_op_delta_add_seg(S(), P(q), P(v), P(t), pitch, 160.0, B, 2, 10, nseg, segs)
        return a, b, msg, lib.pevit_last_error()
    q0 = q.clone()
    for kw, word in ((dict(nseg=17), b"segments outside"), (dict(nseg=0), b"segments outside"), (dict(pitch=128), b"outside the pitch"),
                     (dict(pitch=100), b"multiple of 64"), (dict(B=9), b"cover 8 of 9"), (dict(nseg=2), b"cover 4 of 8")):
        a, b, m1, m2 = both(**kw)
        assert a != 0 and b != 0 and word in m1 and word in m2, (kw, m1, m2)
    segs[1].first = 2                                              # an overlap
    a, b, m1, m2 = both()
    assert a != 0 and b != 0 and b"must tile" in m1 and b"must tile" in m2
    torch.cuda.synchronize()
    assert torch.equal(q, q0) and not bool(out.any())              # nothing was launched


# ---- the engines ------------------------------------------------------------------------------------------------------------------
def two_adapters(arch_name, method):
    arch, _, a = trained(arch_name, method, "bf16")
    _, _, b = trained(arch_name, method, "bf16", classes=7, seed=9)
    return arch, {"a": a, "b": b}


def engine(arch_name, method, ckpts, slots=1):
    from pevit_amd.serving import InferenceEngine
    from pevit_amd.synth import ARCHS
    inf = InferenceEngine(ARCHS[arch_name], method, 10, ARCH_BATCH[arch_name][0], slots=slots)
    inf.load_backbone(backbone(arch_name))
    for name, ck in ckpts.items():
        inf.add_adapter(name, ck)
    return inf


def as_dicts(outs):
    return [{"logits": lo, "features": fe} for lo, fe in outs]


def requests_of(img, counts, names):
    reqs, lo = [], 0
    for c, n in zip(counts, names):
        reqs.append((n, img[lo:lo + c]))
        lo += c
    return reqs


# ---- 2. one segment is predict ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("method", ["kadaptation", "lora"])
@pytest.mark.parametrize("arch_name", list(ARCH_BATCH))
def test_one_segment_is_predict(arch_name, method, fused):
    arch, ckpts = two_adapters(arch_name, method)
    multi, plain = engine(arch_name, method, ckpts, slots=4), engine(arch_name, method, {"a": ckpts["a"]})
    for e in (multi, plain):
        assert e.tune("fused_attn_delta", fused) == 0
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
    # the single-adapter calls on the multi-slot context are the plain context's, bit for bit
    multi.use("a")
    img = images_of(arch, odd, seed=33)
    same_bits(dict(zip(("logits", "features"), multi.predict(img, return_features=True))),
              dict(zip(("logits", "features"), plain.predict(img, return_features=True))))
    same_bits({"features": multi.encode_image(img)}, {"features": plain.encode_image(img)})
    text = torch.nn.functional.normalize(torch.randn((6, arch.embed_dim), generator=torch.Generator().manual_seed(4))).cuda().contiguous()
    keys = ("probs", "logits", "features")
    same_bits(dict(zip(keys, multi.zeroshot(img, text, return_logits=True, return_features=True))),
              dict(zip(keys, plain.zeroshot(img, text, return_logits=True, return_features=True))))
    assert_flags_clear(multi)


# ---- uint8 pixels: the _u8 entry, and native-size requests through the input resize -------------------------------------------------
@pytest.mark.parametrize("arch_name,method", [("tiny-128", "kadaptation"), ("tiny-256", "lora")])
def test_uint8_requests_at_tower_size_and_at_native_size(arch_name, method):
    """Every native-size request is resized into the ONE staging tensor of the engine: a call of several requests must not hand
    the engine the last request's pictures for all of them."""
    from test_gpu_serving import MEAN, STD
    arch, ckpts = two_adapters(arch_name, method)
    multi, plain = engine(arch_name, method, ckpts, slots=2), engine(arch_name, method, ckpts)
    counts = SEGMENTATION[arch_name]
    names = ("a", "b", "a")[:len(counts)]
    n, R = sum(counts), arch.resolution
    g = torch.Generator().manual_seed(8)
    exact = torch.randint(0, 256, (n, 3, R, R), generator=g, dtype=torch.uint8).cuda()
    native = torch.randint(0, 256, (n, 3, R + 12, R + 22), generator=g, dtype=torch.uint8).cuda()
    with pytest.raises(Exception, match="float32"):
        multi.predict_segments(requests_of(exact, counts, names))          # uint8 before set_input_normalization
    for e in (multi, plain):
        e.set_input_normalization(MEAN, STD)

    def check(img):
        got = as_dicts(multi.predict_segments(requests_of(img, counts, names), return_features=True))
        lo = 0
        for i, (c, nm) in enumerate(zip(counts, names)):
            plain.use(nm)
            want = dict(zip(("logits", "features"), plain.predict(img[lo:lo + c], return_features=True)))
            same_bits(got[i], want)
            lo += c
        assert not torch.equal(got[0]["features"][0], got[-1]["features"][-1])
        assert_flags_clear(multi)
    check(exact)                                                            # pevit_predict_segments_u8
    with pytest.raises(Exception):
        multi.predict_segments(requests_of(native, counts, names))          # another size with the resize off
    for e in (multi, plain):
        e.set_input_resize(True)
    check(native)
    # one name per image, native size: the rows of a name are one batch
    row_names = [names[i] for i, c in enumerate(counts) for _ in range(c)][::-1]
    full = multi.predict_mixed(native, row_names)
    for nm in set(row_names):
        rows = [i for i, x in enumerate(row_names) if x == nm]
        plain.use(nm)
        want = plain.predict(native[rows].contiguous())
        same_bits({"logits": full[rows][:, :want.shape[1]].contiguous()}, {"logits": want})
    with pytest.raises(Exception, match="uint8 and float requests"):
        multi.predict_segments([("a", exact[:1]), ("b", images_of(arch, 1))])


# ---- 3. and 4. ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_runs(arch_name, method):
    arch, ckpts = two_adapters(arch_name, method)
    counts = SEGMENTATION[arch_name]
    names = ("a", "b", "a")[:len(counts)]
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


@pytest.mark.parametrize("method", ["kadaptation", "lora"])
@pytest.mark.parametrize("arch_name", list(ARCH_BATCH))
def test_segments_do_not_leak(arch_name, method):
    counts, names, img, runs, alone = mixed_runs(arch_name, method)
    for i, n in enumerate(names):
        same_bits(runs["mixed"][i], runs[n][i])
    # ... and the two adapters differ on the same images, or the comparison shows nothing
    assert not torch.equal(runs["a"][0]["features"], runs["b"][0]["features"])
    assert runs["a"][0]["logits"].shape[1] == 10 and runs["b"][0]["logits"].shape[1] == 7


def plan_floor(arch_name, counts, img):
    """What ``predict`` of a whole batch and of a slice of it differ by on the frozen tower alone (method "none")."""
    _, _, none = trained(arch_name, "none", "bf16")
    e = engine(arch_name, "none", {"n": none})
    e.use("n")
    whole = [x.clone() for x in e.predict(img, return_features=True)]
    floor, lo = 0.0, 0
    for c in counts:
        part = e.predict(img[lo:lo + c], return_features=True)
        floor = max(floor, max_rel(whole[0][lo:lo + c], part[0]), max_rel(whole[1][lo:lo + c], part[1]))
        lo += c
    return floor


@pytest.mark.parametrize("method", ["kadaptation", "lora"])
@pytest.mark.parametrize("arch_name", list(ARCH_BATCH))
def test_segments_are_their_own_batches(arch_name, method):
    counts, names, img, runs, alone = mixed_runs(arch_name, method)
    floor = plan_floor(arch_name, counts, img)
    gate = FLOOR_C * floor
    dist = [max(max_rel(runs["mixed"][i][k], alone[i][k]) for k in ("logits", "features")) for i in range(len(counts))]
    print(f"{arch_name} {method}: segments {counts} slots {names}: plan floor {floor:.3e}, gate {gate:.3e}, distances "
          + ", ".join(f"{d:.3e}" for d in dist))
    for i, d in enumerate(dist):
        assert d <= gate, (i, d, gate)
        if gate == 0.0:
            same_bits(runs["mixed"][i], alone[i])
    # a batch is not the sum of its segments: the whole batch under one adapter differs from the segments of that adapter
    plain = engine(arch_name, method, {"a": two_adapters(arch_name, method)[1]["a"]})
    plain.use("a")
    whole = plain.predict(img)
    assert not torch.equal(whole[:counts[0]], runs["a"][0]["logits"]) or counts[0] == len(img)


# ---- 5. interleaving, poison, no panel-building launch -----------------------------------------------------------------------------
@pytest.mark.parametrize("arch_name,method", [("tiny-128", "kadaptation"), ("tiny-256", "lora"), ("tiny-n257", "kadaptation")])
def test_interleaved_with_single_adapter_calls_and_self_contained_under_poison(arch_name, method):
    arch, ckpts = two_adapters(arch_name, method)
    counts = SEGMENTATION[arch_name]
    names = ("a", "b", "a")[:len(counts)]
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
    assert_flags_clear(Q)
    for a, b in zip(first, again):
        same_bits(b, a)
    # poison: P is filled with NaN bytes before every call, Q keeps the leftovers of whatever ran before
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
    # the slots are loaded: overwrite the f32 sources of the panels (not the delta bias, not the head, which are read in place)
    assert sorted(PP._slot_names) == ["a", "b"]
    want = as_dicts(PP.predict_segments(reqs, return_features=True))
    n_loads = []
    PP._load_slot = lambda slot, name: n_loads.append(name)
    E, L = arch.width, arch.layers
    for n in ("a", "b"):
        p = PP._adapters[n]["params"]
        if method == "lora":
            p[:PP.n_tower].fill_(float("nan"))
        else:
            p[:4096].fill_(float("nan"))
            for l in range(L):
                p[4096 + 5 * E * l:4096 + 5 * E * l + 4 * E].fill_(float("nan"))
    got = as_dicts(PP.predict_segments(reqs, return_features=True))
    for g, w in zip(got, want):
        same_bits(g, w)
    assert not n_loads
    assert_flags_clear(PP)


def test_predict_mixed_is_predict_per_name():
    arch, ckpts = two_adapters("tiny-128", "kadaptation")
    multi, plain = engine("tiny-128", "kadaptation", ckpts, slots=2), engine("tiny-128", "kadaptation", ckpts)
    img = images_of(arch, 8, seed=88)
    names = ["b", "a", "b", "b", "a", "a", "a", "b"]
    full = multi.predict_mixed(img, names)
    assert full.shape == (8, 10)
    for n, width in (("a", 10), ("b", 7)):
        rows = [i for i, x in enumerate(names) if x == n]
        plain.use(n)
        want = plain.predict(img[rows].contiguous())
        same_bits({"logits": full[rows][:, :width].contiguous()}, {"logits": want})
        assert bool((full[rows][:, width:] == float("-inf")).all())


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_any_launch(lib):
    from pevit_amd import _lib
    arch, ckpts = two_adapters("tiny-128", "kadaptation")
    multi, plain = engine("tiny-128", "kadaptation", ckpts, slots=4), engine("tiny-128", "kadaptation", ckpts)
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
    with pytest.raises(_lib.PevitError, match="exceeds max_batch"):
        multi.predict_segments([("a", images_of(arch, 9, seed=6))])
    with pytest.raises(_lib.PevitError, match="slots"):
        plain.predict_segments([("a", img)])
    torch.cuda.synchronize()
    assert torch.equal(multi.workspace, before) and not bool(out.any())        # nothing was launched
    assert_flags_clear(multi)
    again = multi.predict_segments([("a", img[:3]), ("b", img[3:])])
    for g, w in zip(again, good):
        same_bits({"logits": g}, {"logits": w})
    # dropping a resident adapter empties its slot; adding one under a resident name too
    multi.drop("b")
    assert multi._slot_names[:2] == ["a", None]
    multi.add_adapter("a", ckpts["b"])
    assert multi._slot_names[:2] == [None, None]
    plain.use("b")
    same_bits({"logits": multi.predict_segments([("a", img)])[0]}, {"logits": plain.predict(img)})
