// MFMA fragment helpers shared by the kernel files: one definition of every small device function that the attention, adapter
// and low-rank kernels use to feed v_mfma_f32_16x16x32_bf16 (D[i][j] = sum_k A[i][k] B[k][j]; lane l = (m = l & 15, g = l >> 4)
// holds row / column m and the k-slots 8g..8g+7 of an operand, and column m, rows 4g..4g+3 of the accumulator).
// Paths that the tests require to agree bit for bit (fused and two-kernel attention, tn_gemm64 and its in-launch twin, the
// production and the f32-verify kernels) agree because they call the SAME functions here.
#pragma once
#include "common.h"
#include "kernels.h"

__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// 16-byte row fragment: row `row` of a row-major [*, stride] bf16 matrix, elements 32*s+8*g..+7
__device__ __forceinline__ bf16x8 rowfrag(const bf16* base, size_t stride, int row, int s, int g) {
    return load_bf16x8(base + (size_t)row * stride + 32 * s + 8 * g);
}

// ---- attention tiles: row-major LDS tiles [tokens][LD] of 64-wide head rows --------------------------------------------------
// LD = 64: unpadded 128-byte rows, the 16-byte chunks of a row XOR-swizzled by the row (chunk c of row r sits at
// c ^ ((r >> 1) & 7)); any other LD: padded rows, no swizzle, and the address keeps its plain base + immediate form (written
// through the XOR with a zero swizzle, hipcc emits different address arithmetic).  attention.hip states why both exist.
template <int LD>
__device__ __forceinline__ int att_swz(int r) { return LD == 64 ? (r >> 1) & 7 : 0; }
// 16-byte row fragment of an LDS tile: row `row`, elements 32*s+8*g..+7
template <int LD>
__device__ __forceinline__ bf16x8 ldsfrag(const bf16* Ys, int row, int s, int g) {
    if constexpr (LD == 64) return *reinterpret_cast<const bf16x8*>(Ys + row * LD + 8 * ((4 * s + g) ^ att_swz<LD>(row)));
    else return *reinterpret_cast<const bf16x8*>(Ys + row * LD + 32 * s + 8 * g);
}
// 16-byte piece `c` of row `y` of an LDS tile (staging writes)
template <int LD>
__device__ __forceinline__ bf16x8* ldschunk(bf16* Ys, int y, int c) {
    return reinterpret_cast<bf16x8*>(Ys + y * LD + 8 * (c ^ att_swz<LD>(y)));
}

// Fragment of the TRANSPOSE of a row-major tile Ys[y][LD] (LDS), output row m -> d = 16*(m>>2) + 4*dt + (m&3), with gfx950's
// transposing read (ds_read_b64_tr_b16): in each 16-lane
// group, lane 4j+q passes the address of 4 consecutive d of token-row j, and lane i receives, as element j, element i&3
// of the piece addressed by lane 4j + (i>>2) (measured: scripts/probe_tr_b16.hip).  Lane 4j+q therefore points at
// Ys[32s + 4g + j][16q + 4dt ..+3], and lane m ends up with d = 16*(m>>2) + 4*dt + (m&3) for the tokens 32s+4g+0..3
// (second read: +16 tokens) -- no transposed copy in LDS, no scattered 2-byte writes.
__device__ __forceinline__ bf16x8 tr_pair(const bf16* src, int stride16) {
    typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(src));
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(src + stride16));
    bf16x8 o;
    o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = lo[3];
    o[4] = hi[0]; o[5] = hi[1]; o[6] = hi[2]; o[7] = hi[3];
    return o;
}
template <int LD>
__device__ __forceinline__ bf16x8 tfrag_tr(const bf16* Ys, int dt, int s, int lane) {
    const int m = lane & 15, g = lane >> 4;
    const int R = 32 * s + 4 * g + (m >> 2);                     // (row R + 16 has the same swizzle)
    if constexpr (LD == 64) return tr_pair(Ys + R * LD + 8 * ((2 * (m & 3) + (dt >> 1)) ^ att_swz<LD>(R)) + 4 * (dt & 1), 16 * LD);
    else return tr_pair(Ys + R * LD + 16 * (m & 3) + 4 * dt, 16 * LD);
}
// The same read with the plain column map, for the token-contracted products G = X^T Y: fragment of the transpose of a row-major
// LDS tile [token][LD]; lane (m, g) gets column col0 + m for the tokens 32ks + 4g + 0..3 and 32ks + 16 + 4g + 0..3
template <int LD>
__device__ __forceinline__ bf16x8 trfrag(const bf16* tile, int ks, int col0, int lane) {
    const int m = lane & 15, g = lane >> 4;
    return tr_pair(tile + (32 * ks + 4 * g + (m >> 2)) * LD + col0 + 4 * (m & 3), 16 * LD);
}

// the four accumulators of a lane's 16 consecutive d (tfrag_tr's row order), scaled, as two 16-byte stores
__device__ __forceinline__ void store16(bf16* dst, const f32x4 o[4], float scale) {
    bf16x8 a, b;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            a[dt * 4 + r] = f2bf(o[dt][r] * scale);
            b[dt * 4 + r] = f2bf(o[dt + 2][r] * scale);
        }
    store_bf16x8(dst, a);
    store_bf16x8(dst + 8, b);
}

// f32 -> bf16 hi + bf16 lo (hi + lo carries 16 bits of the mantissa): the f32 operand of a bf16 MFMA as two fragments
__device__ __forceinline__ void split_bf16v(const float4 a, const float4 b, bf16x8& hi, bf16x8& lo) {
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        hi[i] = f2bf(v[i]);
        lo[i] = f2bf(v[i] - bf2f(hi[i]));
    }
}

// ---- the flat addressing of the attention-site adapters (lowrank.hip states it) ---------------------------------------------
// reference row rr = n*B + b -> batch-major row b*N + n
__device__ __forceinline__ int row_of_ref(int rr, int B, int N) {
    const int n = rr / B, b = rr - n * B;
    return b * N + n;
}
// address of the 64-element head row that holds flat elements [rr*E + e0, +64) of dDelta (T = bf16, or float in verify.hip)
template <typename T>
__device__ __forceinline__ const T* ddelta_slab(const T* dqkv, int ld, int col0, int rr, int e0, int E, int H, int N) {
    const int c = (int)(((long long)rr * E + e0) >> 6);
    const int bh = c / N, n = c - bh * N;
    const int b = bh / H, h = bh - b * H;
    return dqkv + ((size_t)b * N + n) * ld + col0 + h * 64;
}

// The segment that owns workgroup `wg` of a segmented attention-site launch (kernels.h: SegTable), and the workgroup's index inside
// it.  Static indices and selects only (a dynamic index would copy the table to scratch), and everything here is uniform over the
// workgroup.  What the gfx950 build gives: no scratch in any instance; delta_add_kernel keeps the picked values in SGPRs, the two
// attn_fwd_delta_kernel instances spill 68 / 98 SGPRs into VGPR lanes (160 VGPRs against 154, still 3 waves per SIMD).
struct SegPick {
    int first, count, tcol, wg;
    const bf16* q16; const float* bias;
};
__device__ __forceinline__ SegPick seg_pick(const SegTable& sg, int wg) {
    SegPick p{sg.first[0], sg.count[0], sg.tcol[0], wg, sg.q16[0], sg.bias[0]};
#pragma unroll
    for (int s = 1; s < PEVIT_MAX_SEGMENTS; ++s) {
        const bool in = s < sg.nseg && wg >= sg.wg0[s];
        p.first = in ? sg.first[s] : p.first;
        p.count = in ? sg.count[s] : p.count;
        p.tcol = in ? sg.tcol[s] : p.tcol;
        p.wg = in ? wg - sg.wg0[s] : p.wg;
        p.q16 = in ? sg.q16[s] : p.q16;
        p.bias = in ? sg.bias[s] : p.bias;
    }
    return p;
}

// sum over the 8 row-lanes of a wave that hold the same 16-byte column piece (thread = (row tid >> 3, piece tid & 7))
__device__ __forceinline__ float rowlane_sum(float v) {
    v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
    return v;
}
