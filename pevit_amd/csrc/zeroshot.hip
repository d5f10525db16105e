// The zero-shot head of CLIP (the reference's clip_zeroshot_evaluator.py:16-20): for every image row b
//   s_b        = scale / max(||feat_b||_2, 1e-12)            (the eps clamp of F.normalize)
//   logit[b][c] = s_b * <feat_b, text_c>
//   prob[b][:]  = softmax(logit[b][:])                        (row maximum subtracted)
// in ONE launch, exact f32 on the f32 matrix instruction like the classifier head (stem_head.hip) -- no bf16 rounding anywhere.
//
// feat [B][D] f32, text_cd [C][D] f32 (class-major, one unit vector per row: both operands contiguous along k), probs / logits
// [B][C] f32.  One workgroup of eight waves per 16 image rows.  The 16 rows are staged once in LDS (padded by one 16-byte slot per
// row), their sums of squares taken on the way.  Wave w owns the class tiles w, w + 8, ... (16 classes each, at most 8 tiles = 32
// accumulator registers) and walks all of K itself, so no contraction is ever combined across waves.  Text rows come from global
// memory with 16-byte loads: lane (m, g) of a tile reads k = 32 ch + 8 g .. + 7 of class m for chunk ch -- the four lanes of a class
// take one whole 128-byte line -- and its u-th value feeds the u-th MFMA of the chunk (the contraction order is free as long as
// both operands agree).  All loads of chunk ch + 1 are issued before the MFMAs of chunk ch; no load sits inside a bounds branch --
// classes past C and k past D read a clamped address, and the feature side of such a k is zero.  A workgroup streams all of text
// (up to 4 MB) through one CU, and that stream is its time: 77 us at C = 1000, D = 512, the same with four waves and half the
// bytes in flight (profiles/zeroshot.md); the MFMAs alone would take 27 us.
//
// Every reduction runs in one fixed order that depends on D and C only: the sum of squares (32 lanes per row, each over its own
// 16-byte pieces in ascending k, then a butterfly), the contraction (ascending chunks), the row maximum and the row sum (a wave's
// tiles in ascending order, a butterfly over the tile's 16 class lanes, then the eight waves in wave order through LDS).  None of
// it depends on B or on where a row sits in its workgroup, so a row's outputs are bit-identical alone and inside any batch.
#include "kernels.h"

constexpr int ZS_ROWS = 16;                          // image rows per workgroup
constexpr int ZS_WAVES = 8;
constexpr int ZS_THREADS = 64 * ZS_WAVES;
constexpr int ZS_PAD = 4;                            // floats between the LDS rows: one 16-byte slot
constexpr int ZS_MAX_D = 1024, ZS_MAX_C = 1024;
constexpr int ZS_LDS_MAX = ZS_ROWS * (ZS_MAX_D + ZS_PAD) * 4;

// butterflies over LANES neighbouring lanes (xor < LANES stays inside the group): every lane ends with the same bits
template <int LANES>
__device__ __forceinline__ float zs_sum(float v) {
#pragma unroll
    for (int o = 1; o < LANES; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float zs_max16(float v) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// NT = class tiles per wave (1, 2, 4 or 8: the smallest that covers ceil(C / 16) tiles with eight waves)
template <int NT>
__global__ __launch_bounds__(ZS_THREADS) void zeroshot_head_kernel(ZeroshotArgs a) {
    extern __shared__ __align__(16) float zs_feat[];          // [ZS_ROWS][D + ZS_PAD]
    __shared__ float s_scale[ZS_ROWS];
    __shared__ float s_max[ZS_WAVES][ZS_ROWS];
    __shared__ float s_sum[ZS_WAVES][ZS_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, m = lane & 15, g = lane >> 4;
    const int D = a.D, C = a.C, B = a.B, LD = D + ZS_PAD;
    const int b0 = blockIdx.x * ZS_ROWS;

    // ---- stage the 16 feature rows: thread (row = tid >> 5, j = tid & 31) takes the 16-byte pieces j, j + 32, ... of its row
    {
        const int row = tid >> 5, j = tid & 31;
        const bool rok = b0 + row < B;
        const float* src = a.feat + (size_t)(rok ? b0 + row : B - 1) * D;
        float ss = 0.f;
        for (int c4 = j; 4 * c4 < D; c4 += 32) {
            float4 v = *reinterpret_cast<const float4*>(src + 4 * c4);
            if (!rok) v = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(zs_feat + row * LD + 4 * c4) = v;
            ss = fmaf(v.x, v.x, ss); ss = fmaf(v.y, v.y, ss); ss = fmaf(v.z, v.z, ss); ss = fmaf(v.w, v.w, ss);
        }
        ss = zs_sum<32>(ss);
        if (j == 0) s_scale[row] = a.scale / fmaxf(sqrtf(ss), 1e-12f);
    }
    __syncthreads();

    // ---- logits: acc[t][r] = <feat row 4g + r, text class 16 (wid + 8t) + m>
    int toff[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int cls = 16 * (wid + ZS_WAVES * t) + m;
        toff[t] = (cls < C ? cls : C - 1) * D;
    }
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nch = (D + 31) >> 5;
    float4 cur0[NT], cur1[NT];
    {
        const int k = 8 * g < D ? 8 * g : 0;           // (D % 8 == 0: a lane's 8 values are inside the row or all past it)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            cur0[t] = *reinterpret_cast<const float4*>(a.text + toff[t] + k);
            cur1[t] = *reinterpret_cast<const float4*>(a.text + toff[t] + k + 4);
        }
    }
    for (int ch = 0; ch < nch; ++ch) {
        float4 nxt0[NT], nxt1[NT];
        {
            const int chn = ch + 1 < nch ? ch + 1 : ch;
            const int kn = 32 * chn + 8 * g;
            const int k = kn < D ? kn : 0;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                nxt0[t] = *reinterpret_cast<const float4*>(a.text + toff[t] + k);
                nxt1[t] = *reinterpret_cast<const float4*>(a.text + toff[t] + k + 4);
            }
        }
        const int k = 32 * ch + 8 * g;
        const bool kok = k < D;
        const float* fp = zs_feat + m * LD + (kok ? k : 0);
        float4 f0 = *reinterpret_cast<const float4*>(fp), f1 = *reinterpret_cast<const float4*>(fp + 4);
        if (!kok) f0 = f1 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(f0.x, cur0[t].x, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(f0.y, cur0[t].y, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(f0.z, cur0[t].z, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(f0.w, cur0[t].w, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(f1.x, cur1[t].x, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(f1.y, cur1[t].y, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(f1.z, cur1[t].z, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(f1.w, cur1[t].w, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NT; ++t) { cur0[t] = nxt0[t]; cur1[t] = nxt1[t]; }
    }

    // ---- scale; the row maximum: this wave's tiles in order, the 16 class lanes, then the eight waves in wave order
    float sc[4], mx[4];
    bool rowok[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        sc[r] = s_scale[4 * g + r];
        rowok[r] = b0 + 4 * g + r < B;
        mx[r] = -INFINITY;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int cls = 16 * (wid + ZS_WAVES * t) + m;
        const bool cok = cls < C;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float l = sc[r] * acc[t][r];
            acc[t][r] = l;
            if (cok) mx[r] = fmaxf(mx[r], l);
            if (a.logits && cok && rowok[r]) a.logits[(size_t)(b0 + 4 * g + r) * C + cls] = l;
        }
    }
    if (!a.probs) return;           // (uniform over the grid)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        mx[r] = zs_max16(mx[r]);
        if (m == 0) s_max[wid][4 * g + r] = mx[r];
    }
    __syncthreads();
    float sum[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 4 * g + r;
        float v = s_max[0][row];
#pragma unroll
        for (int w = 1; w < ZS_WAVES; ++w) v = fmaxf(v, s_max[w][row]);
        mx[r] = v;
        sum[r] = 0.f;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const bool cok = 16 * (wid + ZS_WAVES * t) + m < C;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float e = cok ? expf(acc[t][r] - mx[r]) : 0.f;
            acc[t][r] = e;
            sum[r] += e;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        sum[r] = zs_sum<16>(sum[r]);
        if (m == 0) s_sum[wid][4 * g + r] = sum[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 4 * g + r;
        float v = s_sum[0][row];
#pragma unroll
        for (int w = 1; w < ZS_WAVES; ++w) v += s_sum[w][row];
        sum[r] = v;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int cls = 16 * (wid + ZS_WAVES * t) + m;
        if (cls < C) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (rowok[r]) a.probs[(size_t)(b0 + 4 * g + r) * C + cls] = acc[t][r] / sum[r];
        }
    }
}

// the limits of the kernel, checked on the host before any launch (also by the context entries, before they run the tower)
int pevit_zeroshot_check(const ZeroshotArgs& a) {
    if (!a.feat || !a.text) { pevit_set_error("zeroshot_head: null feature or text pointer"); return -1; }
    if (!a.probs && !a.logits) { pevit_set_error("zeroshot_head: both outputs are null (give probs, logits or both)"); return -1; }
    if (a.B < 1) { pevit_set_error("zeroshot_head: batch %d must be at least 1", a.B); return -1; }
    if (a.C < 1 || a.C > ZS_MAX_C) { pevit_set_error("zeroshot_head: %d classes outside [1, %d]", a.C, ZS_MAX_C); return -1; }
    if (a.D < 8 || a.D > ZS_MAX_D || a.D % 8) {
        pevit_set_error("zeroshot_head: feature width %d must be a multiple of 8 in [8, %d]", a.D, ZS_MAX_D); return -1;
    }
    if ((reinterpret_cast<size_t>(a.feat) | reinterpret_cast<size_t>(a.text)) & 15) {
        pevit_set_error("zeroshot_head: feat and text_cd must be 16-byte aligned"); return -1;
    }
    return 0;
}

template <int NT>
static int zs_launch(const ZeroshotArgs& a, hipStream_t s) {
    if (reserve_lds<zeroshot_head_kernel<NT>, ZS_LDS_MAX>("zeroshot_head_kernel")) return -1;
    const size_t lds = (size_t)ZS_ROWS * (a.D + ZS_PAD) * 4;
    hipLaunchKernelGGL(zeroshot_head_kernel<NT>, dim3(ceil_div(a.B, ZS_ROWS)), dim3(ZS_THREADS), lds, s, a);
    LAUNCH_OK("zeroshot_head_kernel");
    return 0;
}

int pevit_launch_zeroshot_head(const ZeroshotArgs& a, hipStream_t s) {
    if (pevit_zeroshot_check(a)) return -1;
    const int per_wave = ceil_div(ceil_div(a.C, 16), ZS_WAVES);
    if (per_wave <= 1) return zs_launch<1>(a, s);
    if (per_wave <= 2) return zs_launch<2>(a, s);
    if (per_wave <= 4) return zs_launch<4>(a, s);
    return zs_launch<8>(a, s);
}
