// gemm_skinny_kernel: the few-row family of gemm.hip (GemmPlan::path 6).  bf16 operands only.
#include "gemm_device.h"

namespace {
// ---------------------------------------------------------------------------------------------------------------------
// Few-row long-K products (M <= 128, K >= 1536: c_proj forward and c_fc backward on the class-token rows of the last block):
// 6 tiles of 128x128 for 256 CUs.  Stream-K gives such a tile two workgroups that walk 24 k-tiles each behind a two-stage
// ring (31 us for 0.6 GFLOP), and is switched off under data parallelism (its consumers WAIT for their producers, which must
// therefore be resident).  Here: 128x64 tiles, the K range cut into a few slices of ~12 k-tiles, one workgroup per
// (tile, slice) with a FOUR-stage ring and exact vmcnt waits; the 128x64 f32 partial goes to a slab (write-through stores) and
// the workgroup that draws the LAST ticket of its tile adds the slabs in slice order -- a fixed order, so the result does not
// depend on who arrives last -- and runs the epilogue.  Nobody waits for anybody: no residency requirement.
// Bounds (measured, profiles/NOTES_gemm.md (r03_gemm_experiments) 5c): one CU moves ~60 GB/s, so both the k-walk of a workgroup and the
// slabs its tile's finisher re-reads must stay at a few hundred KB: 16 slices of 3 k-tiles made the finisher read 1 MB (27 us).
// Slabs and ticket words are the stream-K workspace (GemmParams::sk_slab / sk_flag; tickets return to 0).
template <int EPI>
__global__ __launch_bounds__(256, 1) void gemm_skinny_kernel(GemmParams p, int tiles_n, int nslices, int ksl) {
    constexpr int NW = 4, WN = 2, BM = 128, BN = 64, BK = 64, S = 4;
    constexpr int ROWB = 128, CH = 8, RPP = 8;
    constexpr int A_BYTES = BM * ROWB, B_BYTES = BN * ROWB, STAGE_BYTES = A_BYTES + B_BYTES;
    constexpr int PA = BM / RPP / NW, PB = BN / RPP / NW, KS = BK / 16, NPW = PA + PB;     // pieces per wave per k-tile
    constexpr int SLAB = BM * BN;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ unsigned ticket;
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // wave w: rows 32w .. 32w+31, all 64 columns
    const int tile = blockIdx.x / nslices, slice = blockIdx.x - tile * nslices;
    const int tm = tile / tiles_n, tn = tile - tm * tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    const int nk = p.K / BK;
    const int k0 = slice * ksl, n = min(nk, k0 + ksl) - k0;               // this slice: k-tiles [k0, k0 + n)
    const char* a_src[PA];
    const char* b_src[PB];
#pragma unroll
    for (int i = 0; i < PA; ++i) {
        const int row = (wid * PA + i) * RPP + lane / CH;
        const int chunk = (lane % CH) ^ ((row >> 1) & (CH - 1));
        int ar = m0 + row; ar = ar < p.M ? ar : p.M - 1;
        a_src[i] = reinterpret_cast<const char*>(p.A + (size_t)ar * p.lda) + chunk * 16 + (size_t)k0 * 128;
    }
#pragma unroll
    for (int i = 0; i < PB; ++i) {
        const int row = (wid * PB + i) * RPP + lane / CH;
        const int chunk = (lane % CH) ^ ((row >> 1) & (CH - 1));
        int br = n0 + row; br = br < p.Nb ? br : p.Nb - 1;
        b_src[i] = reinterpret_cast<const char*>(p.B) + (size_t)br * p.ldb * 2 + chunk * 16 + (size_t)k0 * 128;
    }
    auto issue_tile = [&](int kt) {
        char* st = smem + (kt & (S - 1)) * STAGE_BYTES;
#pragma unroll
        for (int i = 0; i < PA; ++i) glds16(a_src[i] + kt * 128, st + (wid * PA + i) * 1024);
#pragma unroll
        for (int i = 0; i < PB; ++i) glds16(b_src[i] + kt * 128, st + A_BYTES + (wid * PB + i) * 1024);
    };
#pragma unroll
    for (int kt = 0; kt < S - 1; ++kt)
        if (kt < n) issue_tile(kt);
    const int frow = lane & 31, fswz = (frow >> 1) & (CH - 1), fhalf = lane >> 5;
    f32x16 acc[WN];
#pragma unroll
    for (int j = 0; j < WN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
    for (int kt = 0; kt < n; ++kt) {
        // k-tile kt has landed when at most the younger requested ones (up to kt + S - 2) are in flight
        const int after = min(n - 1, kt + S - 2) - kt;
        if (after >= 2) wait_vmcnt<2 * NPW>(); else if (after == 1) wait_vmcnt<NPW>(); else wait_vmcnt<0>();
        __syncthreads();                                      // ... for every wave; and stage (kt - 1) % S is free again
        if (kt + S - 1 < n) issue_tile(kt + S - 1);
        const char* sa = smem + (kt & (S - 1)) * STAGE_BYTES;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int coff = (((ks * 2 + fhalf) ^ fswz) << 4);
            const bf16x8 af = *reinterpret_cast<const bf16x8*>(sa + (wid * 32 + frow) * ROWB + coff);
#pragma unroll
            for (int j = 0; j < WN; ++j) {
                const bf16x8 bfr = *reinterpret_cast<const bf16x8*>(sa + A_BYTES + (j * 32 + frow) * ROWB + coff);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bfr, acc[j], 0, 0, 0);
            }
        }
    }
    if (nslices > 1) {
        // ---- publish this slice's partial, draw a ticket; the last arriver of the tile sums all slabs in slice order
        float* slab = p.sk_slab + (size_t)blockIdx.x * SLAB;
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 v = {acc[j][4 * q], acc[j][4 * q + 1], acc[j][4 * q + 2], acc[j][4 * q + 3]};
                sk_store16_sc1(slab + ((((wid * WN + j) * 4 + q) * 64 + lane) << 2), v);
            }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) ticket = __hip_atomic_fetch_add(p.sk_flag + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (ticket != (unsigned)(nslices - 1)) return;        // block-uniform
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        if (threadIdx.x == 0) __hip_atomic_store(p.sk_flag + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next launch
        f32x4 part[6][WN][4];                                 // all slabs requested before the first add
        const float* base = p.sk_slab + (size_t)tile * nslices * SLAB;
#pragma unroll
        for (int sl = 0; sl < 6; ++sl)
            if (sl < nslices) {
#pragma unroll
                for (int j = 0; j < WN; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        part[sl][j][q] = *reinterpret_cast<const f32x4*>(base + (size_t)sl * SLAB + ((((wid * WN + j) * 4 + q) * 64 + lane) << 2));
            }
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
#pragma unroll
        for (int sl = 0; sl < 6; ++sl)
            if (sl < nslices) {
#pragma unroll
                for (int j = 0; j < WN; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc[j][4 * q + r] += part[sl][j][q][r];
            }
    }
    __syncthreads();                                          // every wave is past its LDS reads: stage 0 serves as epilogue scratch
    float* cw = reinterpret_cast<float*>(smem + wid * 4096);
#pragma unroll
    for (int j = 0; j < WN; ++j) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            cw[row * 32 + (lane & 31)] = acc[j][r];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            const int lr = pass * 16 + (lane >> 2);
            const int lc = (lane & 3) * 8;
            const int row = m0 + wid * 32 + lr;
            const int col = n0 + j * 32 + lc;
            const float4 x0 = *reinterpret_cast<const float4*>(cw + lr * 32 + lc);
            const float4 x1 = *reinterpret_cast<const float4*>(cw + lr * 32 + lc + 4);
            if (row < p.M && col < p.N) {
                float v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
                epilogue_store<EPI, bf16>(p, row, col, v);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

template <int EPI>
int launch_skinny(const GemmParams& p, const GemmPlan& pl, hipStream_t s) {
    return launch_kernel<gemm_skinny_kernel<EPI>, 4 * (128 + 64) * 128>(EPI, pl, 256, s, p, pl.tiles_n, pl.nslices, pl.ksl);
}

struct SkinnyFamily {
    template <int EPI, int OPS>
    static int launch(const GemmParams& p, const GemmPlan& pl, hipStream_t s) {
        if constexpr (OPS == 0 && epi_traits(EPI).skinny) return launch_skinny<EPI>(p, pl, s);
        return kNoKernel;
    }
};

}  // namespace

int pevit_gemm::gemm_launch_skinny(int epi, int ops, const GemmParams& p, const GemmPlan& pl, hipStream_t s) {
    return launch_family<SkinnyFamily>(epi, ops, p, pl, s);
}
