// Attention probabilities for MultiheadAttention.forward(..., need_weights=True) (model.py:808-828): the softmax matrix the
// flash-style attention kernels never store.  They keep the row log-sum-exp (attn_fwd / attn_fwd_delta), so P is recomputed
// from the saved operands:
//   S = q k^T          q: the post-delta bf16 q of the engine's head layout (b*H + h, n, 64), already scaled by 1/8 -- exactly the
//                      S of the forward kernel (attention.hip); k: the bf16 keys, same layout
//   P = exp(S - lse)
// and written either as the head mean (B, N, N) f32 -- the sum over the H consecutive b*H + h entries divided by H, as
// `view(bsz, num_heads, N, N).sum(1) / num_heads` does (model.py:821-823) -- or per head (B, H, N, N) f32.  The raw-reshape
// scramble of the attention-site adapters applies to the delta only, which is already inside q: the mapping is the same
// for every method.
//
// One workgroup (4 waves) per (image b, 32-row query tile) loops over the H heads.  Per head and 32x32 (query, key) cell: four
// v_mfma_f32_32x32x16_bf16 over d = 64, operands straight from global memory (row fragments: lane l holds row l&31, d = 8(l>>5)+j of
// each 16-wide k-step, the same map for the q rows (A) and the key rows (B)).  Wave w takes key blocks w, w+4, w+8; in the mean form
// P accumulates in registers over the heads and each output is stored once.  Accumulator map (C/D of 32x32x16): lane l holds key
// column l&31 and query rows (r&3) + 8(r>>2) + 4(l>>5), r = 0..15: one store instruction writes two 128-byte row pieces.
// Out-of-range rows / keys (N not a multiple of 32) read the clamped last row and are never stored.
#include "common.h"
#include "kernels.h"

namespace {

template <bool MEAN, int MAXKB>
__global__ __launch_bounds__(256) void attn_probs_kernel(const bf16* __restrict__ q, const bf16* __restrict__ k,
                                                         const float* __restrict__ lse, float* __restrict__ out, int H, int N, int QT) {
    const int b = blockIdx.x / QT, q0 = (blockIdx.x - b * QT) * 32;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int r32 = lane & 31, half = lane >> 5;
    const int NKB = (N + 31) >> 5;
    const int qrow = min(q0 + r32, N - 1);
    int rows[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) rows[r] = q0 + (r & 3) + 8 * (r >> 2) + 4 * half;
    f32x16 acc[MAXKB];
#pragma unroll
    for (int i = 0; i < MAXKB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    for (int h = 0; h < H; ++h) {
        const size_t bh = (size_t)b * H + h;
        const bf16* qp = q + (bh * N + qrow) * 64 + 8 * half;
        bf16x8 qa[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) qa[s] = load_bf16x8(qp + 16 * s);
        float ls[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) ls[r] = lse[bh * N + min(rows[r], N - 1)];
#pragma unroll
        for (int i = 0; i < MAXKB; ++i) {
            const int kb = wid + 4 * i;
            if (kb >= NKB) break;                       // wave-uniform
            const int col = kb * 32 + r32;
            const bf16* kp = k + (bh * N + min(col, N - 1)) * 64 + 8 * half;
            bf16x8 kf[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) kf[s] = load_bf16x8(kp + 16 * s);
            f32x16 sc;
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[r] = 0.f;
#pragma unroll
            for (int s = 0; s < 4; ++s) sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa[s], kf[s], sc, 0, 0, 0);
            if constexpr (MEAN) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][r] += __expf(sc[r] - ls[r]);
            } else {
                if (col < N) {
                    float* o = out + bh * N * N + col;
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (rows[r] < N) o[(size_t)rows[r] * N] = __expf(sc[r] - ls[r]);
                }
            }
        }
    }
    if constexpr (MEAN) {
        const float fh = (float)H;
#pragma unroll
        for (int i = 0; i < MAXKB; ++i) {
            const int kb = wid + 4 * i;
            const int col = kb * 32 + r32;
            if (kb >= NKB || col >= N) continue;
            float* o = out + (size_t)b * N * N + col;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (rows[r] < N) o[(size_t)rows[r] * N] = acc[i][r] / fh;
        }
    }
}

template <bool MEAN>
int launch(const bf16* q, const bf16* k, const float* lse, float* out, int B, int H, int N, hipStream_t s) {
    const int QT = (N + 31) / 32, nkb = (N + 31) / 32;
    const dim3 grid(B * QT), block(256);
    if (nkb <= 4) hipLaunchKernelGGL((attn_probs_kernel<MEAN, 1>), grid, block, 0, s, q, k, lse, out, H, N, QT);
    else if (nkb <= 8) hipLaunchKernelGGL((attn_probs_kernel<MEAN, 2>), grid, block, 0, s, q, k, lse, out, H, N, QT);
    else hipLaunchKernelGGL((attn_probs_kernel<MEAN, 3>), grid, block, 0, s, q, k, lse, out, H, N, QT);
    LAUNCH_OK("attn_probs_kernel");
    return 0;
}

}  // namespace

int pevit_launch_attn_probs(const AttnArgs& a, hipStream_t s) {
    if (a.N < 1 || a.N > 384) { pevit_set_error("attn_probs: N=%d outside [1,384]", a.N); return -1; }
    if (a.B < 1 || a.H < 1) { pevit_set_error("attn_probs: bad B=%d / H=%d", a.B, a.H); return -1; }
    return a.average ? launch<true>(a.q, a.k, a.lse, a.probs, a.B, a.H, a.N, s) : launch<false>(a.q, a.k, a.lse, a.probs, a.B, a.H, a.N, s);
}
