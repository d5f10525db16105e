// The GEMM planner's interface (gemm_plan.hip): which kernel family runs a product and how.  Host-only and pure -- the planner
// makes no HIP call -- so it is callable without a GPU (pevit_debug_gemm_plan, tests/test_gemm_forms_host.py).  The tables the
// planner and the family units (gemm_tile.hip, gemm_stag8.hip, gemm_split.hip, gemm_streamk.hip, gemm_skinny.hip) both read live
// here, once.
#pragma once
#include "kernels.h"

// hidden, like pevit_host (host_ctx.h): the library exports the C ABI and the launchers, nothing of this
namespace pevit_gemm __attribute__((visibility("hidden"))) {

// m-tiles per band of the tile walk (gemm_device.h tile_origin) and of the stream-K walk the planner lays out (sk_plan)
constexpr int TILE_BAND = 6;

// floats of stream-K workspace a two-slice launch needs: two slabs per tile (ksplit_finish: 8 waves x ceil(WM / 2) fragments x 1024)
constexpr long kz_slab_floats(int wm) { return 2L * 8 * ((wm + 1) / 2) * 1024; }

// residency slots of the stream-K kernel: 2 workgroups per CU, a multiple of 8
inline int sk_slots(int cus) { return min(2 * cus, PEVIT_SK_MAX_SLOTS) & ~7; }

// which kernel families have an instantiation for an epilogue; the launchers instantiate exactly these
struct EpiTraits {
    bool fp8b;     // fp8 B: the frozen-weight products of the block and their dX forms
    bool fp8a;     // fp8 x fp8: the forward frozen products (opt-in weight format "fp8-act")
    bool skinny;   // the few-row kernel
    bool ksplit;   // the k-split, phased k-split and stream-K kernels
};
constexpr EpiTraits epi_traits(int e) {
    const bool gelu = e == EPI_BIAS_GELU || e == EPI_BIAS_GELU_ONLY;      // the inference form runs wherever the saving one does: the same plan
    return {e == EPI_QKV_HEADS || e == EPI_BIAS_RESID_F32 || gelu || e == EPI_DGELU_BF16 || e == EPI_F32 || e == EPI_BF16 || e == EPI_BIAS_F32,
            e == EPI_QKV_HEADS || e == EPI_BIAS_RESID_F32 || gelu || e == EPI_F32,
            e == EPI_BIAS_RESID_F32 || e == EPI_F32 || e == EPI_BF16 || e == EPI_BIAS_RESID_KEEP || gelu || e == EPI_DGELU_BF16,
            e == EPI_BIAS_RESID_F32 || e == EPI_F32 || e == EPI_BF16 || e == EPI_BIAS_RESID_KEEP || e == EPI_PATCH_EMBED};
}

// wgm x wgn waves of wm x wn fragments; wgs = workgroups per CU the LDS and registers are sized for
struct TileConfig { int wgm, wgn, wm, wn, wgs; bool hoist, spread, pipe; };
constexpr TileConfig kConfigs[] = {
    // 4-wave tiles request the next k-tile in one burst: with 2-4 workgroups per CU another workgroup computes while
    // this one sits in its issue slots (in the step: burst 5.59 ms, spread 5.75 ms; profiles/NOTES_gemm.md (r02_gemm_experiments) section 2).  The 8-wave tiles (one workgroup per
    // CU) spread the requests between their MFMAs.
    {2, 2, 2, 2, 2, true, false, false},   // 0: 128x128, 4 waves, 64 KiB, 2 workgroups / CU
    {2, 2, 1, 2, 3, true, false, false},   // 1:  64x128, 4 waves, 48 KiB, 3 workgroups / CU
    {2, 2, 1, 1, 4, false, false, false},  // 2:  64x64,  4 waves, 32 KiB, 4 workgroups / CU (bottleneck products, N <= 64)
    {4, 2, 2, 2, 1, true, true, false},    // 3: 256x128, 8 waves, 96 KiB, 1 workgroup / CU
    {2, 4, 4, 2, 1, false, true, false},   // 4: 256x256, 8 waves, 128 KiB
    {2, 4, 5, 2, 1, false, true, false},   // 5: 320x256, 8 waves, 144 KiB
    {2, 2, 2, 1, 3, true, false, false},   // 6: 128x64,  4 waves, 48 KiB, 3 workgroups / CU
    // software-pipelined twins of 0 and 1 (register double buffer, two k-tiles of LDS-DMA in flight): bit-identical
    // results, measured SLOWER on every shape of the step (c_proj 62.8 vs 54.9 us, 5.48 vs 5.45 ms per step) -- the
    // k-loop is bound by the operand stream, not by the ds_read -> MFMA latency the pipelining removes
    // (profiles/NOTES_gemm.md (r02_gemm_experiments) section 3).  Opt-in through gemm_config / gemm_cfg_longk for measurements only.
    {2, 2, 2, 2, 2, true, false, true},    // 7
    {2, 2, 1, 2, 2, true, false, true},    // 8
};
constexpr int kNumConfigs = sizeof(kConfigs) / sizeof(kConfigs[0]);
constexpr int cfg_bm(int c) { return kConfigs[c].wgm * kConfigs[c].wm * 32; }
constexpr int cfg_bn(int c) { return kConfigs[c].wgn * kConfigs[c].wn * 32; }

// configuration 9 = 160x256 on 1 x 8 waves: only the staggered kernel has it (gemm8_kernel; `allow9`).  It is what fills the
// chip at the reference's own batch of 64 (M = 3200: 240 tiles for c_fc / dGELU where 320x256 has 120).
constexpr int CFG_160x256 = 9;

// the tiles of the 8-wave configurations: 3 (256x128), 4 (256x256), 5 (320x256), CFG_160x256
constexpr int big_bm(int c) { return c == 5 ? 320 : c == CFG_160x256 ? 160 : 256; }
constexpr int big_bn(int c) { return c == 3 ? 128 : 256; }

// stream-K: k-iterations per workgroup (0 = not stream-K), m-tiles per band of its tile walk (sk_plan, gemm_plan.hip)
struct SkPlan { int share, band; };

// Everything one launch needs.  A non-empty err means there is no kernel for the problem.
struct GemmPlan {
    int path = 0;         // kernel family (pevit_gemm_last_path): 1 gemm_kernel, 2 gemm8_kernel, 3 gemm_ksplit_kernel,
                          // 4 gemm_kphase_kernel, 5 gemm_streamk_kernel, 6 gemm_skinny_kernel, 7 gemm_kphase_kernel<..., KZ = true>
    int ops = 0;          // operands: 0 bf16 x bf16, 1 bf16 x fp8 B (on gemm8_kernel with the bf16 tail B2, if set), 2 fp8 x fp8
    int cfg = 0;          // path 1: kConfigs index; path 2: 4, 5, CFG_160x256, or 3 (256x128, two k-steps per phase: measurement)
    int wm = 0;           // paths 3, 4, 7: tile height in 32-row fragments (5: 160x128, 3: 96x128)
    int nl = 0;           // paths 4, 7: LDS-DMA pieces of a k-tile requested in the LOAD section (2 or 8)
    bool stag = false;    // path 3: the two wave groups half an iteration apart
    int tiles = 0, grid = 0, band = 0;   // band: GemmParams::band of paths 2, 3, 4, 7
    SkPlan sk{0, 0};      // path 5: GemmParams::sk_share, sk_band
    int tiles_n = 0, nslices = 0, ksl = 0;   // path 6: 64-column tiles per row of tiles, K slices per tile, k-tiles per slice
    char err[160] = "";
};

// The one place that decides how a product runs: argument checks, then the operand form, then the kernel family and its grid.
// Pure: no HIP calls, no globals (cus = compute units of the device).
GemmPlan plan_gemm(int epi, const GemmParams& p, const GemmTune& t, int cus);

}  // namespace pevit_gemm
