// plan_gemm decides which kernel runs and how; the family units map a plan onto its kernel instantiation.  Host code only: no
// kernel, no HIP runtime call.  (A .hip file all the same, so that the one build rule and bench.py's kernels_hash cover it: which
// kernels a step runs, and so the traffic measured for them, depends on this file.)
#include <cstdarg>
#include <cstdio>

#include "gemm_plan.h"

namespace pevit_gemm __attribute__((visibility("hidden"))) {
namespace {

// band height (m-tiles) that hands every XCD whole bands: tiles / 8 consecutive tile indices per XCD (xcd_remap) = k bands of
// tiles_n * band tiles.  0 = keep TILE_BAND (several rounds, or no even split).
int xcd_band(int tiles, int tiles_n, int grid, const GemmTune& t) {
    if (t.band >= 0) return t.band;
    if (tiles > grid || tiles % 8 || (tiles / 8) % tiles_n) return 0;
    const int per_xcd_m = tiles / 8 / tiles_n;          // m-tiles per XCD
    for (int b = min(per_xcd_m, 8); b >= 1; --b)
        if (per_xcd_m % b == 0) return b;
    return 0;
}

// buffer descriptors address an operand with 31-bit byte offsets: bytes from its base to the end of its last row
constexpr long long kMaxOffset = 1LL << 31;
long long span_bytes(int rows, int ld, int K, int esize) { return ((long long)rows * ld + K) * esize; }
bool fits_31bit(const GemmParams& p, int a_esize, int b_esize) {
    return span_bytes(p.M, p.lda, p.K, a_esize) < kMaxOffset && span_bytes(p.Nb, p.ldb, p.K, b_esize) < kMaxOffset;
}

// Tile shape per problem.  Measured on MI355X (scripts/bench_gemm.py, profiles/NOTES_gemm.md (r02_gemm_experiments)).
// The 8-wave tiles win when their tiling still gives (almost) every CU one tile per round;
// the N = 768 products of the ViT-B step (75 tiles of 256x256) stay on the 4-wave tiles.
int pick_config(const GemmParams& p, const GemmTune& t, bool allow9, int cus) {
    if (t.config >= 0 && t.config < kNumConfigs) return t.config;
    if (t.config == CFG_160x256 && allow9) return CFG_160x256;
    if (p.N <= 64) return 2;
    if (t.big) {
        // rounds of the persistent loop and the fraction of the last round that is filled
        const int cand[4] = {5, 4, 3, CFG_160x256};
        int best = -1; double best_cost = 1e30;
        for (int i = 0; i < (allow9 ? 4 : 3); ++i) {
            const int c = cand[i];
            const int bm = big_bm(c), bn = big_bn(c);
            const long tiles = (long)ceil_div(p.M, bm) * ceil_div(p.N, bn);
            if (tiles * 10 < (long)cus * 7) continue;                 // fewer than 0.7 tiles per CU: leave to the small tiles
            const long rounds = (tiles + cus - 1) / cus;
            // per-CU operand bytes per k-tile (the L1-fill stream) x rounds ~ time of the k-loop
            const double cost = (double)rounds * (bm + bn);
            if (cost < best_cost) { best_cost = cost; best = c; }
        }
        if (best >= 0) {
            // the 128x128 tiling for comparison: 2 workgroups per CU, each streaming 256 rows per k-tile
            const long t128 = (long)ceil_div(p.M, 128) * ceil_div(p.N, 128);
            const double cost128 = (double)((t128 + cus - 1) / cus) * 256.0;
            if (best_cost < cost128 * t.big_bias / 100.0) return best;
        }
    }
    const long t128 = (long)ceil_div(p.M, 128) * ceil_div(p.N, 128);
    if (t128 >= 700) return 0;
    // few-tile problems (the N = E products): 128x128 only when K is long AND its tiles fit the 2 x CUs residency slots in
    // one round -- 300 tiles at ViT-B/32 B=128; at 520 (ViT-L/14, B=32) or 594 (ViT-B/16, B=64) tiles the handful of
    // second-round tiles doubles the kernel time and 64x128 is 1.3-2.7 % faster per step (profiles/NOTES_gemm.md (r02_gemm_experiments) 9)
    return (p.K >= t.kswitch && t128 <= 2L * cus) ? t.cfg_longk : t.cfg_shortk;
}

// Stream-K share (k-iterations per workgroup), 0 = keep the plain tiling.  Measured on the N = 768 products of ViT-B/32
// (scripts/gpu_streamk_sweep.py, profiles/NOTES_gemm.md (r02_gemm_experiments) section 13): the k-loops only get faster when workgroups
// that share an A panel -- TILE_BAND tiles = TILE_BAND * nk iterations apart in the walk -- stay in PHASE (same k at the
// same time), i.e. when the share divides TILE_BAND * nk: otherwise every workgroup streams its own k-slices through the
// XCD's 4 MiB L2 and the kernel becomes fabric-bound (63-75 us against 54 plain).  A share of at least nk / 2 keeps the
// hand-offs at one partial per tile.  K = 3072, 300 tiles: share 32 (450 workgroups), 54.8 -> 43.0 us.  Problems with MORE
// tiles than slots (ViT-B/16 at B = 64: 594, ViT-L/14 at B = 32: 520) were tried with the band chosen along with the share
// (band 7 / share 56, band 9 / share 72): +0.6 % and -3.2 % per step, so they keep the 64x128 tiling.
SkPlan sk_plan(long tiles, int nk, int slots) {
    const long total = tiles * nk;
    const int lo = (int)max((total + slots - 1) / slots, (long)(nk + 1) / 2);
    for (int s = lo; 4 * s <= 3 * nk; ++s)
        if ((TILE_BAND * nk) % s == 0) return SkPlan{s, TILE_BAND};
    return SkPlan{0, 0};
}

// stream-K applies where the heuristic takes the 128x128 tile for a long-K problem with fewer tiles than residency slots
// (the N = E products of ViT-B/32), bf16 B, the five epilogues those products use (c_proj forward with and without the kept MLP output, the
// dX products in f32 / bf16, the patch embedding)
SkPlan streamk_plan(const GemmParams& p, const GemmTune& t, int cfg, int slots) {
    const SkPlan none{0, 0};
    if (!t.streamk || !p.sk_slab || !p.sk_flag || !t.persistent) return none;
    const int tiles_m = ceil_div(p.M, 128);
    const long tiles = (long)tiles_m * ceil_div(p.N, 128);
    const int nk = p.K / 64;
    if (slots < 8) return none;
    if (t.streamk == 2)        // measurement only
        return (t.sk_share && (tiles * nk + t.sk_share - 1) / t.sk_share <= slots) ? SkPlan{t.sk_share, t.sk_band ? t.sk_band : TILE_BAND} : none;
    if (t.config >= 0 || cfg != 0 || t.ablate || nk < 16 || tiles >= slots) return none;
    const SkPlan pl = sk_plan(tiles, nk, slots);
    if (pl.share) return pl;
    return t.streamk == 3 ? SkPlan{nk, TILE_BAND} : none;     // 3: the whole-tile walk through this kernel (measurement)
}

// the 160x128 two-group tile: where the heuristic takes a 4-wave tile for a long-K problem whose 160x128 tiling gives (almost)
// every CU exactly one tile -- the N = E products of ViT-B/32 at B = 128 (240 tiles)
// returns the tile height in fragments: 5 (160x128), 3 (96x128: M = 3200, the reference's own batch of 64, gives 204 tiles where
// 160x128 gives 120), or 0 = not this kernel
int use_ksplit(const GemmParams& p, const GemmTune& t, int cfg, int cus) {
    if (!t.ksplit || t.config >= 0 || (cfg != 0 && cfg != 1) || t.ablate || p.K < t.ksplit_mink) return 0;
    const int chip = cus & ~7;
    const int cand[2] = {5, 3};
    for (int i = 0; i < (t.ksplit_small ? 2 : 1); ++i) {
        const long tiles = (long)ceil_div(p.M, cand[i] * 32) * ceil_div(p.N, 128);
        const long rounds = (tiles + chip - 1) / chip;
        if (t.ksplit == 1 && rounds > 1) continue;          // 2: also problems of several rounds (measurement)
        if (4 * tiles >= 3 * rounds * chip) return cand[i];  // the last round at least 3/4 full on average
    }
    return 0;
}

__attribute__((format(printf, 1, 2))) GemmPlan plan_error(const char* fmt, ...) {
    GemmPlan pl;
    va_list ap; va_start(ap, fmt); vsnprintf(pl.err, sizeof(pl.err), fmt, ap); va_end(ap);
    return pl;
}

GemmPlan plan_gemm8(const GemmParams& p, const GemmTune& t, int cus, int cfg, int ops) {
    GemmPlan pl; pl.path = 2; pl.cfg = cfg; pl.ops = ops;
    const int tiles_n = ceil_div(p.N, big_bn(cfg)); pl.tiles = ceil_div(p.M, big_bm(cfg)) * tiles_n;
    pl.grid = t.persistent && pl.tiles > cus ? cus : pl.tiles;
    pl.band = xcd_band(pl.tiles, tiles_n, pl.grid, t);
    return pl;
}

// paths 3, 4, 7: (wm x 32) x 128 tiles, at most one workgroup per CU; path 7 has two workgroups per tile
GemmPlan plan_split(const GemmParams& p, const GemmTune& t, int cus, int path, int wm) {
    GemmPlan pl; pl.path = path; pl.wm = wm;
    const int tiles_n = ceil_div(p.N, 128); pl.tiles = ceil_div(p.M, wm * 32) * tiles_n;
    pl.grid = min(path == 7 ? 2 * pl.tiles : pl.tiles, cus & ~7);
    pl.band = xcd_band(pl.tiles, tiles_n, min(pl.tiles, pl.grid), t);
    return pl;
}

// the kernel for a checked problem with bf16 or fp8 B: the families in the order they are tried
GemmPlan plan_tiles(const EpiTraits& tr, const GemmParams& p, const GemmTune& t, int cus) {
    const bool bf8 = p.b_fp8;
    const int nk = p.K / 64;
    const int slots = min(sk_slots(cus), p.sk_slots);
    // few-row long-K products on gemm_skinny_kernel: 2-6 slices of ~12 k-tiles, tiles x slices within the slab slots
    if (tr.skinny && !bf8 && t.skinny && t.config < 0 && !t.ablate && p.sk_slab && p.sk_flag && p.M <= t.skinny_maxm && p.N >= 64 &&
        nk >= t.skinny_mink) {
        GemmPlan pl; pl.path = 6;
        pl.tiles_n = ceil_div(p.N, 64); pl.tiles = ceil_div(p.M, 128) * pl.tiles_n;
        pl.nslices = t.skinny_slices > 0 ? min(6, max(1, t.skinny_slices)) : nk < 24 ? 1 : min(6, max(2, (nk + 6) / 12));
        // a slot holds 128x128 floats: two of these slabs; tickets: one word per tile
        if ((long)pl.tiles * pl.nslices <= 2L * slots && pl.tiles <= slots) {
            pl.ksl = ceil_div(nk, pl.nslices); pl.grid = pl.tiles * pl.nslices;
            return pl;
        }
    }
    // the staggered 8-wave kernel, where the operands are addressable with 31-bit byte offsets
    const bool stag = t.stagger && !(t.ablate & 12) && fits_31bit(p, 2, bf8 ? 1 : 2);
    const int cfg = pick_config(p, t, stag, cus);
    if (stag && (cfg == 5 || cfg == 4 || cfg == CFG_160x256 || (cfg == 3 && t.stagger >= 2)))
        return plan_gemm8(p, t, cus, cfg, bf8 ? 1 : 0);
    if (tr.ksplit && !bf8) {
        const int kwm = use_ksplit(p, t, cfg, cus);
        if (kwm && t.ksplit_stagger == 2) {
            // two workgroups per 160x128 tile, half of K each (opt-in): where those tiles fill at most half the chip and each slice still
            // walks >= 16 k-tiles (M = 3200, N = 768, K >= 2048: three products per layer at batch 64), one ticket + two slabs per tile
            const long t160 = (long)ceil_div(p.M, 160) * ceil_div(p.N, 128);
            const int chip = cus & ~7;
            if (t.kz2 && p.sk_slab && p.sk_flag && 2 * t160 <= chip && 4 * t160 >= chip && nk >= 32 && t160 <= p.sk_slots &&
                t160 * kz_slab_floats(5) <= (long)p.sk_slots * PEVIT_SK_SLAB_FLOATS && fits_31bit(p, 2, 2)) {
                GemmPlan pl = plan_split(p, t, cus, 7, 5); pl.nl = 8;
                return pl;
            }
            // the phased kernel; beyond 31-bit offsets the alternate-k-tile one.  Requests between the MFMAs (kphase_nl = 2: two in
            // LOAD, the rest behind every second MFMA) win 3 % back to back and lose 0.9 % in the step (28.14 k vs 27.89 k
            // images/s, two pairs; profiles/NOTES_gemm.md (r03_gemm_experiments) section 8)
            GemmPlan pl = plan_split(p, t, cus, fits_31bit(p, 2, 2) ? 4 : 3, kwm);
            pl.nl = t.kphase_nl <= 2 ? 2 : 8; pl.stag = true;
            return pl;
        }
        if (kwm) {
            GemmPlan pl = plan_split(p, t, cus, 3, kwm); pl.stag = kwm == 3 || t.ksplit_stagger;
            return pl;
        }
        const SkPlan sk = streamk_plan(p, t, cfg, slots);
        if (sk.share) {
            GemmPlan pl; pl.path = 5; pl.sk = sk; pl.tiles = ceil_div(p.M, 128) * ceil_div(p.N, 128);
            // every workgroup must be resident: the grid never exceeds the 2-per-CU slots (streamk_plan checked that)
            pl.grid = (int)(((long)pl.tiles * nk + sk.share - 1) / sk.share + 7) & ~7;
            return pl;
        }
    }
    GemmPlan pl; pl.path = 1; pl.ops = bf8 ? 1 : 0; pl.cfg = cfg >= 0 && cfg < kNumConfigs ? cfg : 5;
    const int wgs = kConfigs[pl.cfg].wgs; pl.tiles = ceil_div(p.M, cfg_bm(pl.cfg)) * ceil_div(p.N, cfg_bn(pl.cfg));
    // persistent grid: one workgroup per residency slot (a multiple of 8 keeps XCD affinity), or one
    // per tile when the tiles do not even fill the slots
    pl.grid = t.persistent && pl.tiles > cus * wgs ? cus * wgs : pl.tiles;
    return pl;
}

}  // namespace

// The one place that decides how a product runs: argument checks, then the operand form, then the kernel family and its grid.
// Pure: no HIP calls, no globals (cus = compute units of the device).
GemmPlan plan_gemm(int epi, const GemmParams& p, const GemmTune& t, int cus) {
    if (p.K % 64 != 0 || p.K <= 0) return plan_error("gemm: K=%d must be a positive multiple of 64", p.K);
    if (p.N % 8 != 0) return plan_error("gemm: N=%d must be a multiple of 8", p.N);
    if (p.M <= 0 || p.N <= 0) return plan_error("gemm: empty problem M=%d N=%d", p.M, p.N);
    if ((!p.a_fp8 && (p.lda % 8)) || (p.ldb % (p.b_fp8 ? 16 : 8))) return plan_error("gemm: lda/ldb must be multiples of 8 (16 for fp8 B)");
    // the bf16 tail of an fp8-B problem (B2) is written by gemm8_kernel<.., OPS = 1> only, on its 256-column tiles: the tail starts
    // on a tile boundary and is addressed through B's buffer descriptor, so it lies behind B, within 31 bits of it
    const char* no_tail = "gemm: this problem has no kernel with a bf16 tail (ask pevit_gemm_mixed_ok first)";
    if (p.B2) {
        const long long off = reinterpret_cast<const char*>(p.B2) - reinterpret_cast<const char*>(p.B);
        if (epi != EPI_QKV_HEADS || !p.b_fp8 || p.a_fp8 || p.n_fp8 % 256 || p.K % 128 || off <= 0 ||
            off + span_bytes(p.Nb2, p.ldb2, p.K, 2) >= kMaxOffset)
            return plan_error("%s", no_tail);
    }
    const EpiTraits tr = epi_traits(epi);
    if (p.a_fp8) {
        if (!p.b_fp8 || p.K % 128 != 0 || (p.lda % 16)) return plan_error("gemm: fp8 A needs fp8 B, K %% 128 == 0 and lda %% 16 == 0");
        if (!tr.fp8a) return plan_error("gemm: epilogue %d has no fp8 x fp8 form", epi);
        if (!fits_31bit(p, 1, 1)) return plan_error("gemm (fp8 x fp8): operands beyond 2 GiB");
        // always the staggered kernel's 160x256 tile on 1 x 8 waves: a fragment of the 64-deep instruction is 8 registers per lane,
        // and with two fragment columns per wave (320x256 / 256x256: 160 / 128 accumulator registers + 56 / 48 of fragments)
        // hipcc spills 166 / 26 registers
        return plan_gemm8(p, t, cus, CFG_160x256, 2);
    }
    if (p.b_fp8 && p.K % 128 != 0) return plan_error("gemm: fp8 B needs K=%d to be a multiple of 128", p.K);
    if (p.b_fp8 && !tr.fp8b) return plan_error("gemm: epilogue %d has no fp8-weight form", epi);
    if (epi < EPI_QKV_HEADS || epi > EPI_LAST) return plan_error("gemm: unknown epilogue %d", epi);
    const GemmPlan pl = plan_tiles(tr, p, t, cus);
    if (p.B2 && (pl.path != 2 || big_bn(pl.cfg) != 256)) return plan_error("%s", no_tail);
    return pl;
}

}  // namespace pevit_gemm
