// What the GEMM kernel families share on the device -- the tile walk, the fp8 fragment conversion, the buffer form of the LDS-DMA,
// the slab hand-off store, the end of a k-split tile -- and the one launch helper of their units (gemm_tile.hip, gemm_stag8.hip,
// gemm_split.hip, gemm_streamk.hip, gemm_skinny.hip).  gemm.hip carries the header comment of the family.
#pragma once
#include <type_traits>
#include <utility>

#include "common.h"
#include "kernels.h"
#include "gemm_epilogue.h"
#include "gemm_plan.h"

using namespace pevit_gemm;

namespace {
// measurement bits of GemmParams::dbg; -DGEMM_NO_DBG compiles them out
#ifdef GEMM_NO_DBG
#define GEMM_DBG(p, bit) false
#else
#define GEMM_DBG(p, bit) ((p).dbg & (bit))
#endif

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// tile coordinates of this workgroup.  Order: XCD-contiguous (xcd_remap), and inside that a band
// of TILE_BAND m-tiles is walked n-major, so the tiles an XCD has in flight share TILE_BAND
// A-panels and only a few B-panels (a 128x768 bf16 panel is 192 KiB; the XCD's L2 is 4 MiB).
// GemmParams::band overrides the band height: a one-round launch whose tiles split evenly over the 8 XCDs gives every XCD
// whole bands, so that no A panel is fetched by two private L2s (xcd_band below).
template <int BM, int BN>
__device__ __forceinline__ void tile_origin(const GemmParams& p, int tile, int& m0, int& n0) {
    const int tiles_n = (p.N + BN - 1) / BN;
    const int tiles_m = (p.M + BM - 1) / BM;
    const int t = xcd_remap(tile, tiles_m * tiles_n);
    const int tb = p.band > 0 ? p.band : TILE_BAND;
    const int band = t / (tb * tiles_n), within = t - band * (tb * tiles_n);
    const int mb = min(tb, tiles_m - band * tb);
    const int tn = within / mb, tm = band * tb + (within - tn * mb);
    m0 = tm * BM; n0 = tn * BN;
}

// 8 fp8 codes (two dwords) -> 8 bf16, exact
__device__ __forceinline__ bf16x8 fp8x8_to_bf16(int lo, int hi) {
    const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false);
    const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
    const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false);
    const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
    bf16x8 o;
    o[0] = a[0]; o[1] = a[1]; o[2] = b[0]; o[3] = b[1]; o[4] = c[0]; o[5] = c[1]; o[6] = d[0]; o[7] = d[1];
    return o;
}

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;

typedef __attribute__((address_space(3))) void* lds_void_ptr;

// 16 bytes per lane, buffer form of the LDS-DMA: descriptor {base, bytes} + per-lane byte offset + scalar byte offset.
// Kept in a __device__ function: written inline in the kernel (or in a lambda of it) the HOST pass of hipcc silently drops the
// whole kernel stub (a deferred diagnostic on the builtin's operands that is never printed) and the library fails to load
// with an undefined symbol.
__device__ __forceinline__ void buffer_lds16(const void* base, int bytes, char* lds_wave_base, int voff, int soff) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_ptr)lds_wave_base, 16, voff, soff, 0, 0);
}

// the tile walk of gemm_streamk_kernel (gemm_streamk.hip)
__device__ __forceinline__ void sk_tile_origin(const GemmParams& p, int t, int& m0, int& n0) {
    const int tiles_n = (p.N + 127) / 128, tiles_m = (p.M + 127) / 128, tb = p.sk_band;
    const int band = t / (tb * tiles_n), within = t - band * (tb * tiles_n);
    const int mb = min(tb, tiles_m - band * tb);
    const int tn = within / mb, tm = band * tb + (within - tn * mb);
    m0 = tm * 128; n0 = tn * 128;
}

__device__ __forceinline__ void sk_store16_sc1(float* dst, f32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(dst), "v"(v) : "memory");
}

// The end of a k-split tile, shared by gemm_ksplit_kernel and gemm_kphase_kernel: the two groups' partial sums meet through
// LDS (every wave is past its last k-tile and has no request in flight): fragment f = i * WN + j is FINISHED by group f % 2,
// which receives the other group's partial at hand[((gw * NF + f) * 16 + r) * 64 + lane] and runs that fragment's epilogue.
// SCRATCH_OFF: byte offset of the 4 KiB-per-wave epilogue scratch, behind the hand-off area.
// KZ (round 5): the tile's K range is split over TWO workgroups (slice z = 0, 1).  After the groups' hand-off each wave holds the
// workgroup's sums of the fragments it finishes; it publishes them in the stream-K workspace (slab tile * 2 + z, write-through),
// the workgroup draws a ticket, and the one that arrives LAST adds the other's slab and runs the epilogue -- nobody waits for
// anybody (no residency requirement), and with two slices the sum does not depend on who was last (a + b = b + a).  Returns false
// in the workgroup that arrived first (it has nothing left to do for this tile).
template <int EPI, int WM, int WN, int NWG, int NOWN, int SCRATCH_OFF, bool KZ = false>
__device__ __forceinline__ bool ksplit_finish(const GemmParams& p, char* smem, f32x16 (&acc)[WM][WN], float4 (&rpre)[NOWN][2][2],
                                              float (&bpre)[WN][8], int m0, int n0, int grp, int gw, int wm, int wn, int wid, int lane,
                                              int tile = 0, int z = 0) {
    constexpr bool PRE = (EPI == EPI_BIAS_RESID_F32 || EPI == EPI_BIAS_RESID_KEEP);
    constexpr int NF = WM * WN;
    constexpr int NOWNF = (NF + 1) / 2;                          // fragments a wave finishes at most
    constexpr int SLABF = 2 * NWG * NOWNF * 16 * 64;            // floats a workgroup publishes
    float* hand = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
            if (((i * WN + j) & 1) != grp) {
#pragma unroll
                for (int r = 0; r < 16; ++r) hand[((gw * NF + i * WN + j) * 16 + r) * 64 + lane] = acc[i][j][r];
            }
    __syncthreads();
    if constexpr (KZ) {
        __shared__ unsigned kz_ticket;
        float* mine = p.sk_slab + (size_t)(tile * 2 + z) * SLABF + (size_t)wid * NOWNF * 1024;
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j) {
                if (((i * WN + j) & 1) != grp) continue;
                const int k = (i * WN + j) >> 1;                  // fragment 2k + grp is this wave's k-th (a compile-time index)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] += hand[((gw * NF + i * WN + j) * 16 + r) * 64 + lane];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 v = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
                    sk_store16_sc1(mine + ((k * 4 + q) * 64 + lane) * 4, v);
                }
            }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) kz_ticket = __hip_atomic_fetch_add(p.sk_flag + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (kz_ticket != 1u) return false;                      // workgroup-uniform: the other slice finishes the tile
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        if (threadIdx.x == 0) __hip_atomic_store(p.sk_flag + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next launch
        const float* other = p.sk_slab + (size_t)(tile * 2 + (1 - z)) * SLABF + (size_t)wid * NOWNF * 1024;
        f32x4 part[NOWNF][4];                                    // every piece requested before the first add
#pragma unroll
        for (int kk = 0; kk < NOWNF; ++kk)
#pragma unroll
            for (int q = 0; q < 4; ++q) part[kk][q] = *reinterpret_cast<const f32x4*>(other + ((kk * 4 + q) * 64 + lane) * 4);
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j) {
                if (((i * WN + j) & 1) != grp) continue;
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[i][j][4 * q + r] += part[(i * WN + j) >> 1][q][r];
            }
    }
    static_assert(SCRATCH_OFF >= NWG * NF * 16 * 64 * 4, "epilogue scratch must not overlap the hand-off area");
    // 4 KiB of epilogue scratch per wave behind the hand-off area (launch_ksplit sizes the LDS for it)
    float* cw = reinterpret_cast<float*>(smem + SCRATCH_OFF + wid * 4096);
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            if (((i * WN + j) & 1) != grp) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if constexpr (KZ) cw[row * 32 + (lane & 31)] = acc[i][j][r];      // (the other group's share went in above)
                else cw[row * 32 + (lane & 31)] = acc[i][j][r] + hand[((gw * NF + i * WN + j) * 16 + r) * 64 + lane];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int pass = 0; pass < 2; ++pass) {
                const int lr = pass * 16 + (lane >> 2);
                const int lc = (lane & 3) * 8;
                const int row = m0 + wm * WM * 32 + i * 32 + lr;
                const int col = n0 + wn * WN * 32 + j * 32 + lc;
                const float4 x0 = *reinterpret_cast<const float4*>(cw + lr * 32 + lc);
                const float4 x1 = *reinterpret_cast<const float4*>(cw + lr * 32 + lc + 4);
                if (row < p.M && col < p.N) {
                    float v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
                    if constexpr (PRE) {          // epilogue_store<EPI_BIAS_RESID_*> with the residual and the bias already in registers
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] += bpre[j][e];
                        if constexpr (EPI == EPI_BIAS_RESID_KEEP) store8f(p.outf2 + (size_t)row * p.ldo2 + col, v);
                        const float4 r0 = rpre[(i * WN + j) >> 1][pass][0], r1 = rpre[(i * WN + j) >> 1][pass][1];
                        v[0] += r0.x; v[1] += r0.y; v[2] += r0.z; v[3] += r0.w;
                        v[4] += r1.x; v[5] += r1.y; v[6] += r1.z; v[7] += r1.w;
                        store8f(p.outf + (size_t)row * p.ldo + col, v);
                    } else {
                        epilogue_store<EPI, bf16>(p, row, col, v);
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    return true;
}

// ---- launchers: a plan onto its kernel instantiation
const char* const kFamily[] = {"", "tile", "staggered 8-wave", "k-split", "phased k-split", "stream-K", "few rows", "two K slices per tile"};

// what a family's entry returns when it has no instantiation for (path, epilogue, operand form): pevit_launch_gemm (gemm.hip) turns
// it into the error text.  0 = launched, -1 = the launch failed (error text set).
constexpr int kNoKernel = 1;

// The one launch of every family.  The dynamic-LDS limit of an instantiation is raised by its first launch (lds_limit, common.h).
template <auto KERN, int LDS, typename... Args>
int launch_kernel(int epi, const GemmPlan& pl, int block, hipStream_t stream, Args... args) {
    const hipError_t attr = lds_limit<KERN, LDS>();
    if (attr == hipSuccess) hipLaunchKernelGGL(KERN, dim3(pl.grid), dim3(block), LDS, stream, args...);
    const hipError_t e = attr != hipSuccess ? attr : hipGetLastError();
    if (e != hipSuccess) {
        pevit_set_error("gemm (%s, epi %d): %s failed: %s", kFamily[pl.path], epi, attr ? "raising the dynamic LDS limit" : "kernel launch",
                        hipGetErrorString(e));
        return -1;
    }
    return 0;
}

// A family's launches by operand form and epilogue, EPI_QKV_HEADS (0) .. EPI_LAST.  FAMILY::launch<EPI, OPS> names the family's kernel
// instantiations, gated by epi_traits(EPI), or returns kNoKernel; plan_gemm refused any other epilogue.
template <typename FAMILY, int OPS, int... E>
int launch_epi(int epi, const GemmParams& p, const GemmPlan& pl, hipStream_t s, std::integer_sequence<int, E...>) {
    constexpr int (*table[])(const GemmParams&, const GemmPlan&, hipStream_t) = {&FAMILY::template launch<E, OPS>...};
    return table[epi](p, pl, s);
}
template <typename FAMILY>
int launch_family(int epi, int ops, const GemmParams& p, const GemmPlan& pl, hipStream_t s) {
    constexpr auto epis = std::make_integer_sequence<int, EPI_LAST + 1>{};
    switch (ops) {
        case 2: return launch_epi<FAMILY, 2>(epi, p, pl, s, epis);
        case 1: return launch_epi<FAMILY, 1>(epi, p, pl, s, epis);
        default: return launch_epi<FAMILY, 0>(epi, p, pl, s, epis);
    }
}

}  // namespace

// one entry per family unit: the launch of plan pl (pl.path is the family's) for epilogue epi and operand form ops
namespace pevit_gemm __attribute__((visibility("hidden"))) {
int gemm_launch_tile(int epi, int ops, const GemmParams& p, const GemmPlan& pl, hipStream_t s);      // path 1
int gemm_launch_stag8(int epi, int ops, const GemmParams& p, const GemmPlan& pl, hipStream_t s);     // path 2
int gemm_launch_split(int epi, int ops, const GemmParams& p, const GemmPlan& pl, hipStream_t s);     // paths 3, 4, 7
int gemm_launch_streamk(int epi, int ops, const GemmParams& p, const GemmPlan& pl, hipStream_t s);   // path 5
int gemm_launch_skinny(int epi, int ops, const GemmParams& p, const GemmPlan& pl, hipStream_t s);    // path 6
}  // namespace pevit_gemm
