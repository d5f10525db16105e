// bf16 x {bf16 | fp8-e4m3} -> f32 "NT" GEMM on the CDNA4 matrix cores with fused epilogues.
//
//   C[M,N] = A[M,K] * B[N,K]^T          A, B row-major, K contiguous in both
//
// This one kernel family carries every dense contraction of the ViT block that the
// reference issues as aten::linear / mm: QKV projection (model.py:675),
// out-projection (:816), c_fc / c_proj (:959-961) and their dX-only backward forms
// (the backbone is frozen, so no dW GEMMs exist).  Weights are stored [out][in] exactly
// as the OpenAI checkpoint has them, which is already the K-contiguous "B^T" layout the
// MFMA B-fragment wants; the backward GEMMs use a transposed copy made once at load.
//
// One kernel template, two workgroup geometries:
//   * 4 waves (2x2), tiles 64x64 .. 128x128, 2-4 workgroups per CU: the many-small-tiles regime
//     (N = 768 products of the ViT-B step: 300-600 tiles for 256 CUs);
//   * 8 waves (2x4 / 4x2), tiles 256x128 .. 320x256, ONE workgroup per CU: every k-tile moves
//     (BM+BN)*128 bytes through the CU's L1 for 2*BM*BN*64 flops, half the bytes per flop of the
//     128x128 tile.  The L2 -> LDS operand stream (~23 B/clk/CU, profiles/NOTES_gemm.md (r01_l2_fetch_bound)) is
//     what bounds these GEMMs, so the large tile is the lever wherever the tile count still fills
//     the chip (N >= 2304 at M = 6400).
// Operands are staged HBM->LDS with 16-byte LDS-DMA (global_load_lds), double buffered,
// XOR-swizzled on the *source* side so that the ds_read_b128 fragment reads are bank-conflict
// free (cdna guide T2 / rule 21).  v_mfma_f32_32x32x16_bf16 throughout.
//
// fp8 weights (BASELINE config 5): B holds OCP e4m3 codes with one power-of-two scale per output
// channel.  A k-tile of B is then 64 BYTES per row, half a cache line, so B is staged in
// 128-byte rows = TWO k-tiles at a time (every other iteration; same piece geometry, swizzle and
// LDS footprint as the bf16 path, half the bytes per flop).  The codes are stored k-permuted
// inside every 128-element group (fp8_kperm below) so that one lane's fragments of a k-tile are
// 32 contiguous bytes: two ds_read_b128, then v_cvt_scalef32_pk_bf16_fp8 (exact: e4m3 is a
// subset of bf16) feeds the same bf16 MFMA.  The channel scale multiplies the f32 accumulator in
// the epilogue, which is exact for powers of two: the fp8 path is BIT-IDENTICAL to the bf16 path
// run on the de-quantised weights (tests/test_gpu_fp8.py).
//
// Epilogue: accumulators are transposed through LDS, one 32x32 fragment per wave at a time, so
// that global accesses are 16/32-byte-per-lane row segments.
//
// The family's files: gemm_plan.h / gemm_plan.hip (the pure planner and its tables), gemm_device.h (device helpers the kernels share,
// the launch helper), one unit per kernel family -- gemm_tile.hip (gemm_kernel), gemm_stag8.hip (gemm8_kernel), gemm_split.hip
// (gemm_ksplit_kernel, gemm_kphase_kernel), gemm_streamk.hip, gemm_skinny.hip -- and this one: plan, then the family's entry.
#include "gemm_device.h"

namespace {
thread_local int g_last_path = 0;   // which kernel family the last pevit_launch_gemm OF THIS THREAD took (pevit_debug_last_gemm_path; tests): contexts driven from different threads do not share it

// compute units of the current device, read once (a function-local static: contexts driven from several threads may all ask first)
int num_cus() {
    static const int n = [] {
        int dev = 0, cus = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
        return cus > 0 ? cus : 256;
    }();
    return n;
}

}  // namespace

// a bf16 tail (B2) is only accepted where the plan puts the problem on a gemm8_kernel tile that writes it
bool pevit_gemm_mixed_ok(const GemmParams& p, const GemmTune& t) {
    return p.B2 && !plan_gemm(EPI_QKV_HEADS, p, t, num_cus()).err[0];
}

int pevit_num_cus() { return num_cus(); }
int pevit_gemm_sk_slots() { return sk_slots(num_cus()); }
int pevit_gemm_last_path() { return g_last_path; }

int pevit_launch_gemm(int epi, const GemmParams& p_in, const GemmTune& t, hipStream_t stream) {
    GemmParams p = p_in;
    p.dbg = t.ablate;
    const GemmPlan pl = plan_gemm(epi, p, t, num_cus());
    if (pl.err[0]) { pevit_set_error("%s", pl.err); return -1; }
    int rc = kNoKernel;      // the family's entry names its kernel instantiations; the epilogue's traits keep out those it has no form of
    switch (pl.path) {
        case 1: rc = gemm_launch_tile(epi, pl.ops, p, pl, stream); break;
        case 2: rc = gemm_launch_stag8(epi, pl.ops, p, pl, stream); break;
        case 3: case 4: case 7: rc = gemm_launch_split(epi, pl.ops, p, pl, stream); break;
        case 5: rc = gemm_launch_streamk(epi, pl.ops, p, pl, stream); break;
        case 6: rc = gemm_launch_skinny(epi, pl.ops, p, pl, stream); break;
    }
    if (rc == kNoKernel) {
        pevit_set_error("gemm: no kernel for path %d, epilogue %d, operand form %d", pl.path, epi, pl.ops);   // plan_gemm reads the same traits
        return -1;
    }
    if (rc == 0) g_last_path = pl.path;
    return rc;
}
