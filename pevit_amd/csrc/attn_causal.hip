// Causal softmax attention, forward only, for the CLIP text tower: one (prompt, head) per workgroup.
//
// Reference math: the text transformer's MultiheadAttention with the upper-triangular -inf mask (model.py build_attention_mask):
// query x sees the keys y <= x.  The formulation, the swizzled LD = 64 LDS tiles and the numerics are those of attn_fwd_kernel
// (attention.hip): Z^T[y][x] = sum_d K[y][d] Q[x][d] puts a whole softmax row of one query into one 16-lane column, the bf16-rounded
// probabilities feed the P V product straight from the accumulator registers, and the row sum is taken over those rounded values.
// No log-sum-exp: nothing differentiates through the text tower.
//
// N <= 128 (CLIP: 77), so K and V of the head (<= 16 KB each) are LDS-resident and the scores of a 16-query tile stay in registers.
// Causality:
//   * query tile xt walks the key tiles 0..xt only: tiles entirely above the diagonal are never computed (xt is wave-uniform, so
//     the bound is a scalar branch around whole MFMA groups), and the P V product walks the 32-key pairs 0..xt/2;
//   * inside the tiles that are computed the mask is a select (key <= query ? score : -3e38), never a branch -- on the tiles
//     below the diagonal it selects the score everywhere, on the diagonal tile it cuts the upper triangle.  A masked score gives
//     exp(-3e38 - m) = 0 exactly, so a row depends on the keys at or before it and on nothing else, bit for bit.
// Wave balance: tile i costs i + 1 key tiles, so wave w takes the PAIR of tiles (w, nxt - 1 - w): nxt + 1 key tiles for every
// wave (the middle tile of an odd count is a half share for the last wave).  One wave per 32 tokens of the instance (KT32 waves:
// 3 at N = 77, tiles (0,4) (1,3) (2)), so no wave is left without a tile.
// Loads: every K / V piece of a thread and the Q fragments of BOTH its tiles are requested before the first LDS write, and no load
// sits inside a bounds branch -- rows beyond N re-read row N - 1; V's are zeroed by a select, K's are masked by causality (a key
// beyond N lies after every valid query).
#include "common.h"
#include "kernels.h"
#include "mfma_frag.h"

namespace {

constexpr int CA_LD = 64;      // swizzled 128-byte rows (mfma_frag.h att_swz)

template <int KT32>
__global__ __launch_bounds__(64 * KT32) void attn_causal_fwd_kernel(const bf16* __restrict__ q, const bf16* __restrict__ k,
                                                                    const bf16* __restrict__ v, bf16* __restrict__ out, int ldo,
                                                                    int H, int N) {
    constexpr int NPAD = 32 * KT32, NW = KT32, NT = 64 * NW;
    __shared__ __attribute__((aligned(16))) bf16 Ks[NPAD * CA_LD];      // rows beyond N: whatever row N - 1 holds (never selected)
    __shared__ __attribute__((aligned(16))) bf16 Vs[NPAD * CA_LD];      // rows beyond N zero
    const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
    const bf16* qh = q + (size_t)bh * N * 64;
    const bf16* kh = k + (size_t)bh * N * 64;
    const bf16* vh = v + (size_t)bh * N * 64;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, g = lane >> 4, c16 = lane & 15;
    const int nxt = (N + 15) >> 4;
    // this wave's two query tiles (the second one only where it is another tile than the first)
    const int xt0 = wid, xt1 = nxt - 1 - wid;
    bf16x8 qf[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int xs = max(min(16 * (t ? xt1 : xt0) + c16, N - 1), 0);
        qf[t][0] = rowfrag(qh, 64, xs, 0, g);
        qf[t][1] = rowfrag(qh, 64, xs, 1, g);
    }
    constexpr int IT = NPAD * 8 / NT;      // = 4 pieces of K and of V per thread
    {
        bf16x8 kk[IT], vv[IT];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int idx = threadIdx.x + NT * it, y = idx >> 3, c = idx & 7;
            const int ys = y < N ? y : N - 1;
            kk[it] = load_bf16x8(kh + (size_t)ys * 64 + 8 * c);
            vv[it] = load_bf16x8(vh + (size_t)ys * 64 + 8 * c);
        }
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int idx = threadIdx.x + NT * it, y = idx >> 3, c = idx & 7;
            *ldschunk<CA_LD>(Ks, y, c) = kk[it];
            *ldschunk<CA_LD>(Vs, y, c) = y < N ? vv[it] : zero_bf16x8();
        }
    }
    // vmcnt(0), visible to the compiler: the Q fragments of the second tile were requested ahead of K / V, so they are in by now --
    // without this hipcc waits for them behind the first tile's (conditional) stores, and on gfx950 that wait is a store round trip
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();

#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int xt = t ? xt1 : xt0;
        if (t ? (xt1 <= xt0) : (xt0 > xt1)) continue;      // wave-uniform: the pair's tiles, the middle tile once
        const int xq = 16 * xt + c16;                       // this lane's query (column)
        f32x4 z[2 * KT32];
        float m = -3.0e38f;
#pragma unroll
        for (int yt = 0; yt < 2 * KT32; ++yt) {
            f32x4 acc = {-3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f};
            if (yt <= xt) {
                acc = f32x4{0.f, 0.f, 0.f, 0.f};
                acc = mfma16(ldsfrag<CA_LD>(Ks, 16 * yt + c16, 0, g), qf[t][0], acc);
                acc = mfma16(ldsfrag<CA_LD>(Ks, 16 * yt + c16, 1, g), qf[t][1], acc);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = 16 * yt + 4 * g + r;
                    acc[r] = key <= xq ? acc[r] : -3.0e38f;
                    m = fmaxf(m, acc[r]);
                }
            }
            z[yt] = acc;
        }
        m = fmaxf(m, __shfl_xor(m, 16, 64));
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        float l = 0.f;
        bf16x8 pf[KT32];
#pragma unroll
        for (int s = 0; s < KT32; ++s) {
            pf[s] = zero_bf16x8();
            if (2 * s <= xt) {
#pragma unroll
                for (int half = 0; half < 2; ++half)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float p = __expf(z[2 * s + half][r] - m);
                        // the row sum uses the bf16-rounded probabilities that the PV product sees
                        const bf16 pb = f2bf(p);
                        l += bf2f(pb);
                        pf[s][half * 4 + r] = pb;
                    }
            }
        }
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        f32x4 o[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KT32; ++s) {
            if (2 * s <= xt) {
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) o[dt] = mfma16(tfrag_tr<CA_LD>(Vs, dt, s, lane), pf[s], o[dt]);
            }
        }
        if (xq < N) store16(out + ((size_t)b * N + xq) * ldo + h * 64 + 16 * g, o, 1.0f / l);
    }
}

template <int KT32>
int launch_causal(const AttnArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((attn_causal_fwd_kernel<KT32>), dim3(a.B * a.H), dim3(64 * KT32), 0, s, a.q, a.k, a.v, a.out, a.ldo, a.H, a.N);
    LAUNCH_OK("attn_causal_fwd_kernel");
    return 0;
}

}  // namespace

int pevit_launch_attn_fwd_causal(const AttnArgs& a, hipStream_t s) {
    if (a.N < 1 || a.N > 128) { pevit_set_error("attn_fwd_causal: tokens per prompt N=%d outside [1,128]", a.N); return -1; }
    if (a.B < 1 || a.H < 1) { pevit_set_error("attn_fwd_causal: bad B / H %d / %d", a.B, a.H); return -1; }
    if (a.ldo % 8 || a.ldo < 64 * a.H) { pevit_set_error("attn_fwd_causal: ldo %d must be a multiple of 8 and at least 64 H", a.ldo); return -1; }
    if (!a.q || !a.k || !a.v || !a.out) { pevit_set_error("attn_fwd_causal: null argument"); return -1; }
    // the smallest instance whose 32 * KT32 rows hold the N tokens: then every wave owns at least one query tile
    if (a.N <= 32) return launch_causal<1>(a, s);
    if (a.N <= 64) return launch_causal<2>(a, s);
    if (a.N <= 96) return launch_causal<3>(a, s);
    return launch_causal<4>(a, s);
}
