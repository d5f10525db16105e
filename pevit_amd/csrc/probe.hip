// The linear probe's head on CACHED feature rows (evaluation/full_model_finetune.py with FREEZE_IMAGE_BACKBONE: nothing below the
// head trains, so every image goes through the tower once per checkpoint and every step after that is head-only work):
//   x_b      = feat[index[b]]                                              (gather; labels / targets are indexed the same way)
//   xhat     = BatchNorm1d(D, affine=False)(x)                             (batch statistics, or the running ones in eval mode)
//   logits   = s * (xhat W^T + bias)                                       (s = exp(logit_scale), frozen: full_model_finetune.py:156)
//   loss     = CrossEntropyLoss / BCEWithLogitsLoss (mean), dW, db, and torch.optim.SGD's update of W and bias
// as TWO launches with no waiting between workgroups, in place of bn_fwd -> small_gemm -> ce_loss -> small_gemm -> sgd.
//
// Launch 1, probe_fwd_kernel<true>: one workgroup per 32 batch rows.  EVERY workgroup recomputes the batch statistics of all D
// columns from the gathered rows (one read: the two-pass form on 32 rows held in registers, trips and row groups joined by the
// pairwise update; at B <= 128 these are L2 hits) in one fixed order -- thread (column quad q, row group g) takes rows g, g + G, ...
// in ascending order, the G groups are joined in group order -- so all
// workgroups hold the same bits and nothing has to cross between them.  Workgroup 0 alone updates the running statistics (PyTorch's
// rule, as bn_fwd_kernel).  The workgroup's 32 normalised rows are staged in LDS (one 16-byte pad per row: conflict-free 16-byte
// reads) and written out for launch 2.  Wave w owns the class tiles w, w + 4, ... (32 classes each) and walks all of K itself on
// v_mfma_f32_32x32x2_f32 (exact f32), so no contraction is combined across waves and a row's logits depend on D and C only; W comes
// from global memory with 16-byte loads, a trip of eight chunks (32 MFMAs) ahead of its MFMAs.  Behind one barrier wave w takes rows w, w + 4, ... of the
// tile: ce_kernel's semantics / bce_loss_kernel's arithmetic per row, dlogits (times s: the chain rule through the scale), the row's loss term.
//
// Launch 2, probe_update_kernel: one workgroup per 32x32 tile of W, small_gemm_kernel's contraction over the batch (wave w takes
// the row pairs w, w + 4, ...; the four partial tiles are added in wave order).  The tile owners of feature column 0 also own the
// bias (db = column sums of dlogits).  Gradients are WRITTEN (not accumulated: no zero-fill runs before), and with `update` the
// owned elements take sgd_kernel's expressions.  Workgroup (0, 0) finishes the loss mean in loss_mean_kernel's order.
//
// No load sits inside a bounds branch: rows, classes and chunks past the end read a clamped address and are masked afterwards.
// Index values are clamped to [0, rows) on the device, so a bad index reads a wrong row, never out of bounds.
#include "kernels.h"

constexpr int PB_ROWS = 32;                          // batch rows per workgroup of launch 1
constexpr int PB_THREADS = 256;
constexpr int PB_PAD = 4;                            // floats between the LDS rows: one 16-byte slot
constexpr int PB_MAX_D = 1024, PB_MAX_C = 1024;
constexpr int PB_LDS_MAX = (PB_ROWS * (PB_MAX_D + PB_PAD) + 2 * PB_MAX_D) * 4;
constexpr int PB_IDX_LDS = 2048;                    // batch slots whose source row is staged in LDS (the rest re-read the index list)
constexpr int PB_CE_IGNORE = -100;                   // torch.nn.CrossEntropyLoss's default ignore_index (stem_head.hip: CE_IGNORE)

namespace {

// the source row of batch slot b (b inside [0, B)): index[b], or row0 + b without an index list; clamped to the matrix
__device__ __forceinline__ long pb_row(const ProbeArgs& a, int b) {
    const long r = a.index ? (long)a.index[b] : a.row0 + b;
    return r < 0 ? 0 : (r >= a.rows ? a.rows - 1 : r);
}
__device__ __forceinline__ float4 pb_add(float4 s, float4 v) { return make_float4(s.x + v.x, s.y + v.y, s.z + v.z, s.w + v.w); }
// ... from the staged copy where there is one (rows < 2^31: checked on the host)
__device__ __forceinline__ long pb_row(const ProbeArgs& a, const int* s_row, int b) {
    return b < PB_IDX_LDS ? (long)s_row[b] : pb_row(a, b);
}
// Mean and centred sum of squares of columns 4q .. 4q+3 over this thread's row group (rows g, g + G, ...) with ONE read of the batch:
// a trip holds PB_SU rows in registers (128 registers; their source rows come from LDS, so the loads of a trip depend on
// nothing), takes the trip's mean and then its centred squares FROM THE REGISTERS -- the two-pass form, without the second read,
// which was 7 us of a 41 us launch at B = 128 -- and joins the trips by the pairwise update of Chan, Golub and LeVeque:
//   n = na + nb, d = mb - ma, mean = ma + d * nb / n, M2 = M2a + M2b + d * d * na * nb / n
constexpr int PB_SU = 32;
struct PbMoments { float4 mean, m2; float n; };
__device__ __forceinline__ void pb_join(PbMoments& x, float4 mb, float4 m2b, float nb) {
    if (nb == 0.f) return;
    const float n = x.n + nb, wb = nb / n, wab = x.n * wb;
    const float4 d = make_float4(mb.x - x.mean.x, mb.y - x.mean.y, mb.z - x.mean.z, mb.w - x.mean.w);
    x.mean = make_float4(x.mean.x + d.x * wb, x.mean.y + d.y * wb, x.mean.z + d.z * wb, x.mean.w + d.w * wb);
    x.m2 = make_float4(x.m2.x + m2b.x + d.x * d.x * wab, x.m2.y + m2b.y + d.y * d.y * wab, x.m2.z + m2b.z + d.z * d.z * wab,
                       x.m2.w + m2b.w + d.w * d.w * wab);
    x.n = n;
}
__device__ __forceinline__ PbMoments pb_colstats(const ProbeArgs& a, const int* s_row, int q, int g, int G) {
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    PbMoments x{zero, zero, 0.f};
    for (int b = g; b < a.B; b += PB_SU * G) {
        float4 v[PB_SU];
#pragma unroll
        for (int u = 0; u < PB_SU; ++u) {
            const int bb = min(b + u * G, a.B - 1);
            v[u] = *reinterpret_cast<const float4*>(a.feat + pb_row(a, s_row, bb) * a.D + 4 * q);
        }
        float4 sum = zero;
        float cnt = 0.f;
#pragma unroll
        for (int u = 0; u < PB_SU; ++u) {
            const bool ok = b + u * G < a.B;
            if (!ok) v[u] = zero;
            cnt += ok ? 1.f : 0.f;
            sum = pb_add(sum, v[u]);
        }
        const float4 m = make_float4(sum.x / cnt, sum.y / cnt, sum.z / cnt, sum.w / cnt);
        float4 sq = zero;
#pragma unroll
        for (int u = 0; u < PB_SU; ++u) {
            float4 t = make_float4(v[u].x - m.x, v[u].y - m.y, v[u].z - m.z, v[u].w - m.w);
            t = make_float4(t.x * t.x, t.y * t.y, t.z * t.z, t.w * t.w);
            if (b + u * G >= a.B) t = zero;
            sq = pb_add(sq, t);
        }
        pb_join(x, m, sq, cnt);
    }
    return x;
}

// NS = registers per lane for one row of logits (64 classes each): the smallest of 2, 4, 8, 16 that covers C
template <bool STEP, int NS>
__global__ __launch_bounds__(PB_THREADS) void probe_fwd_kernel(ProbeArgs a) {
    extern __shared__ __align__(16) float pb_lds[];           // xs [32][D + 4] | mean [D] | rstd [D]
    __shared__ __align__(16) float part[2][PB_THREADS * 4];   // mean | centred squares, [row group][D]: G * D <= 1024
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, li = lane & 31, lk = lane >> 5;
    const int D = a.D, C = a.C, B = a.B, LD = D + PB_PAD, nq = D >> 2;
    float* xs = pb_lds;
    float* mean_s = xs + PB_ROWS * LD;
    float* rstd_s = mean_s + D;
    const int b0 = blockIdx.x * PB_ROWS;
    // the step reads the source row of EVERY batch slot (statistics, label count): staged once.  A predict workgroup reads its
    // own 32 rows only, once each, straight from the index list -- of 10,000 rows it would otherwise stage 2048 it never uses
    __shared__ int s_row[STEP ? PB_IDX_LDS : 1];
    if (STEP) {
        for (int b = tid; b < min(B, PB_IDX_LDS); b += PB_THREADS) s_row[b] = (int)pb_row(a, b);
        __syncthreads();
    }

    // ---- the first W chunks of this wave's first class tile are requested before anything else: they depend on nothing the
    // statistics produce, and W was last written by another CU (the previous step's update), so its first touch is a trip to memory
    constexpr int CU = 8;                                      // chunks per trip; the next trip's W is requested before this trip's MFMAs
    const int ntile = (C + 31) >> 5, nch = D >> 3;
    float4 cur[CU];
    {
        const int j = 32 * wid + li;
        const float* wp = a.W + (size_t)(j < C ? j : C - 1) * D + 4 * lk;
#pragma unroll
        for (int u = 0; u < CU; ++u) cur[u] = *reinterpret_cast<const float4*>(wp + 8 * min(u, nch - 1));
    }

    // ---- the statistics of all D columns
    if (STEP && a.training) {
        const int G = PB_THREADS / nq;                        // row groups (nq <= 256)
        const int q = tid % nq, g = min(tid / nq, G - 1);     // (threads past the last group repeat it and write nothing)
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        const PbMoments mine = pb_colstats(a, s_row, q, g, G);
        if (tid / nq < G) {
            *reinterpret_cast<float4*>(part[0] + g * D + 4 * q) = mine.mean;
            *reinterpret_cast<float4*>(part[1] + g * D + 4 * q) = mine.m2;
        }
        __syncthreads();
        if (tid < nq) {
            // the G groups are joined in group order (group i holds the rows i, i + G, ...: ceil((B - i) / G) of them): every
            // workgroup walks the same order and ends with the same bits
            PbMoments x{zero, zero, 0.f};
            for (int i = 0; i < G; ++i)
                pb_join(x, *reinterpret_cast<const float4*>(part[0] + i * D + 4 * q), *reinterpret_cast<const float4*>(part[1] + i * D + 4 * q),
                        (float)((B - i + G - 1) / G));
            const float fB = (float)B;
            const float4 mean = x.mean, qq = x.m2;
            const float var[4] = {qq.x / fB, qq.y / fB, qq.z / fB, qq.w / fB};      // biased: used for normalisation
            const float mu[4] = {mean.x, mean.y, mean.z, mean.w}, q4[4] = {qq.x, qq.y, qq.z, qq.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int d = 4 * q + e;
                mean_s[d] = mu[e];
                rstd_s[d] = rsqrtf(var[e] + 1e-5f);
                if (blockIdx.x == 0) {
                    const float unbiased = B > 1 ? q4[e] / (float)(B - 1) : var[e];
                    a.running_mean[d] = 0.9f * a.running_mean[d] + 0.1f * mu[e];
                    a.running_var[d] = 0.9f * a.running_var[d] + 0.1f * unbiased;
                }
            }
        }
    } else {
        for (int d = tid; d < D; d += PB_THREADS) {
            mean_s[d] = a.running_mean[d];
            rstd_s[d] = rsqrtf(a.running_var[d] + 1e-5f);
        }
    }
    __syncthreads();

    // ---- normalise the workgroup's rows: thread (row = tid >> 3, j = tid & 7) takes the 16-byte pieces j, j + 8, ... of its row
    {
        const int row = tid >> 3, j = tid & 7;
        const int b = b0 + row;
        const bool rok = b < B;
        const int bs = rok ? b : B - 1;
        const float* src = a.feat + (STEP ? pb_row(a, s_row, bs) : pb_row(a, bs)) * D;
#pragma unroll 8
        for (int c4 = j; c4 < nq; c4 += 8) {
            const float4 v = *reinterpret_cast<const float4*>(src + 4 * c4);
            const float4 m = *reinterpret_cast<const float4*>(mean_s + 4 * c4);
            const float4 r = *reinterpret_cast<const float4*>(rstd_s + 4 * c4);
            float4 x = make_float4((v.x - m.x) * r.x, (v.y - m.y) * r.y, (v.z - m.z) * r.z, (v.w - m.w) * r.w);
            if (!rok) x = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(xs + row * LD + 4 * c4) = x;
            if (STEP && rok) *reinterpret_cast<float4*>(a.xhat + (size_t)b * D + 4 * c4) = x;
        }
    }
    __syncthreads();

    // ---- logits: wave w owns class tiles w, w + 4, ...; lane (li, lk) holds k = 8 c + 4 lk .. + 3 of chunk c for both operands
    for (int t = wid; t < ntile; t += 4) {
        const int j = 32 * t + li;
        const bool jok = j < C;
        const float* wp = a.W + (size_t)(jok ? j : C - 1) * D + 4 * lk;
        const float* xp = xs + li * LD + 4 * lk;
        const float bv = a.bias[jok ? j : C - 1];
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        // (behind the last trip of a tile nxt holds the first chunks of the wave's NEXT tile)
        const int jn = 32 * (t + 4) + li;
        const float* wpn = a.W + (size_t)(jn < C ? jn : C - 1) * D + 4 * lk;
        for (int cb = 0; cb < nch; cb += CU) {
            float4 nxt[CU], x4[CU];
            const bool last = cb + CU >= nch;
#pragma unroll
            for (int u = 0; u < CU; ++u)
                nxt[u] = *reinterpret_cast<const float4*>(last ? wpn + 8 * min(u, nch - 1) : wp + 8 * min(cb + CU + u, nch - 1));
#pragma unroll
            for (int u = 0; u < CU; ++u) {
                const bool cok = cb + u < nch;
                x4[u] = *reinterpret_cast<const float4*>(xp + 8 * (cok ? cb + u : 0));
                if (!cok) x4[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < CU; ++u) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x4[u].x, cur[u].x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x4[u].y, cur[u].y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x4[u].z, cur[u].z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x4[u].w, cur[u].w, acc, 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < CU; ++u) cur[u] = nxt[u];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int b = b0 + (r & 3) + 8 * (r >> 2) + 4 * lk;
            if (b < B && jok) a.logits[(size_t)b * C + j] = a.scale * (acc[r] + bv);
        }
    }
    if (!STEP) return;
    __syncthreads();                                          // the tile's logits, written by all four waves, are read back below

    // ---- loss and dlogits: wave w takes rows w, w + 4, ... of the tile, RG rows at a time: every value of a group is requested before
    // the first reduction, and the butterflies of the RG rows run interleaved (one row at a time a row was twelve dependent
    // cross-lane exchanges, 1 us: 8.6 us of the launch for the eight rows of a wave)
    constexpr int RG = NS <= 2 ? 8 : (NS <= 4 ? 4 : (NS <= 8 ? 2 : 1));
    const bool bce = a.targets != nullptr;
    float nvalid = 0.f;                                       // cross-entropy: the non-ignored rows of the whole batch
    if (!bce) {
        for (int b = lane; b < B; b += 64) nvalid += a.labels[pb_row(a, s_row, b)] != PB_CE_IGNORE ? 1.f : 0.f;
        nvalid = wave_sum(nvalid);
        if (blockIdx.x == 0 && tid == 0) a.rowloss[B] = nvalid;      // (launch 2 divides the loss sum by it)
    }
    const float nall = (float)B * (float)C, inv_n = 1.f / nall;
    const float nanv = __builtin_nanf("");
    int cc[NS];
    bool ok[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u) { ok[u] = lane + 64 * u < C; cc[u] = ok[u] ? lane + 64 * u : C - 1; }
    for (int r0 = wid; r0 < PB_ROWS; r0 += 4 * RG) {
        float v[RG][NS], y[RG][NS], red[RG], sum[RG];
        int64_t lab64[RG];
#pragma unroll
        for (int i = 0; i < RG; ++i) {
            const int b = min(b0 + r0 + 4 * i, B - 1);
            const long src = pb_row(a, s_row, b);
#pragma unroll
            for (int u = 0; u < NS; ++u) {
                v[i][u] = a.logits[(size_t)b * C + cc[u]];
                y[i][u] = bce ? a.targets[(size_t)src * C + cc[u]] : 0.f;
            }
            lab64[i] = bce ? 0 : a.labels[src];
        }
        if (bce) {
#pragma unroll
            for (int i = 0; i < RG; ++i) {
                const int b = b0 + r0 + 4 * i;
                red[i] = 0.f;
#pragma unroll
                for (int u = 0; u < NS; ++u) {
                    const float x = v[i][u];
                    const float e = expf(-fabsf(x));
                    const float l = fmaxf(x, 0.f) - x * y[i][u] + log1pf(e);
                    const float sg = (x >= 0.f ? 1.f : e) * __builtin_amdgcn_rcpf(1.f + e);
                    red[i] += ok[u] ? l : 0.f;
                    if (ok[u] && b < B) a.dlogits[(size_t)b * C + lane + 64 * u] = a.scale * ((sg - y[i][u]) * inv_n);
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1)
#pragma unroll
                for (int i = 0; i < RG; ++i) red[i] += __shfl_xor(red[i], o, 64);
#pragma unroll
            for (int i = 0; i < RG; ++i) {
                const int b = b0 + r0 + 4 * i;
                if (lane == 0 && b < B) a.rowloss[b] = red[i];
            }
            continue;
        }
        // softmax as e / sum(e) and the row loss as log(sum e) - (x_label - max): the large row maximum never meets the small
        // log-sum in one rounding (m + log(s) costs every probability of the row 1 ulp OF THE MAXIMUM: 4e-6 at the CLIP scale,
        // which the updated parameters' gate of 1e-6 sees through the momentum buffer)
#pragma unroll
        for (int i = 0; i < RG; ++i) {
            red[i] = -3.0e38f;
#pragma unroll
            for (int u = 0; u < NS; ++u) if (ok[u]) red[i] = fmaxf(red[i], v[i][u]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int i = 0; i < RG; ++i) red[i] = fmaxf(red[i], __shfl_xor(red[i], o, 64));
#pragma unroll
        for (int i = 0; i < RG; ++i) {
            sum[i] = 0.f;
#pragma unroll
            for (int u = 0; u < NS; ++u) { y[i][u] = ok[u] ? expf(v[i][u] - red[i]) : 0.f; sum[i] += y[i][u]; }     // (y: the row's e)
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int i = 0; i < RG; ++i) sum[i] += __shfl_xor(sum[i], o, 64);
#pragma unroll
        for (int i = 0; i < RG; ++i) {
            const int b = b0 + r0 + 4 * i;
            const bool ignored = lab64[i] == PB_CE_IGNORE, bad = !ignored && (lab64[i] < 0 || lab64[i] >= C);
            const int lab = (int)lab64[i];
            float at = 0.f;
#pragma unroll
            for (int u = 0; u < NS; ++u) {
                const float g = (y[i][u] / sum[i] - (lane + 64 * u == lab ? 1.f : 0.f)) / nvalid;
                if (ok[u] && b < B) a.dlogits[(size_t)b * C + lane + 64 * u] = ignored ? 0.f : (bad ? nanv : a.scale * g);
                at = (lab >> 6) == u ? v[i][u] : at;
            }
            at = __shfl(at, lab & 63, 64);                     // the label's logit: held by lane lab % 64
            if (lane == 0 && b < B) a.rowloss[b] = ignored ? 0.f : (bad ? nanv : logf(sum[i]) - (at - red[i]));
        }
    }
}

// dW[c][d] = sum_b dlogits[b][c] xhat[b][d], db[c] = sum_b dlogits[b][c]; torch.optim.SGD on the owned tile (sgd_kernel's expressions)
__global__ __launch_bounds__(PB_THREADS) void probe_update_kernel(ProbeArgs a) {
    __shared__ float red[3][64][17];
    __shared__ float rs[3][64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, li = lane & 31, lk = lane >> 5;
    const int D = a.D, C = a.C, B = a.B;
    const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;       // class tile, feature tile
    const int i = i0 + li, j = j0 + li;
    const bool iok = i < C, jok = j < D;
    const float* ap = a.dlogits + (iok ? i : 0);                // A(i, k) = dlogits[k][i]
    const float* bp = a.xhat + (jok ? j : 0);                   // B(k, j) = xhat[k][j]
    // parameters and momentum of the 16 owned elements (wave 0 finishes the tile): requested first, from clamped addresses, so that
    // they arrive under the contraction instead of behind it
    float p[16], mo[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int oi = min(i0 + (r & 3) + 8 * (r >> 2) + 4 * lk, C - 1);
        const size_t e = (size_t)oi * D + (jok ? j : 0);
        p[r] = a.pW[e];
        mo[r] = a.mW[e];
    }
    const float pb0 = a.pB[iok ? i : 0], mb0 = a.mB[iok ? i : 0];
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float rsum = 0.f;
    // wave w takes the row pairs w, w + 4, ...; 8 pairs are requested ahead of their MFMAs
    const int npairs = (B + 1) / 2;
    constexpr int PU = 8;
    for (int pb = wid; pb < npairs; pb += 4 * PU) {
        float av[PU], bv[PU];
#pragma unroll
        for (int u = 0; u < PU; ++u) {
            const int k = 2 * (pb + 4 * u) + lk;
            const bool kok = pb + 4 * u < npairs && k < B;
            const int kc = kok ? k : 0;
            const float x = ap[(size_t)kc * C], w = bp[(size_t)kc * D];
            av[u] = kok && iok ? x : 0.f;
            bv[u] = kok && jok ? w : 0.f;
        }
#pragma unroll
        for (int u = 0; u < PU; ++u) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
            rsum += av[u];
        }
    }
    if (wid > 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) red[wid - 1][lane][r] = acc[r];
        rs[wid - 1][lane] = rsum;
    }
    __syncthreads();
    if (wid == 3 && blockIdx.x == 0 && blockIdx.y == 0) {       // the loss mean: one wave, fixed order (loss_mean_kernel)
        float s = 0.f;
        for (int b = lane; b < B; b += 64) s += a.rowloss[b];
        s = wave_sum(s);
        const float n = a.targets ? (float)B * (float)C : a.rowloss[B];      // (the non-ignored rows: counted by launch 1)
        if (lane == 0) a.loss[0] = s / n;
    }
    if (wid != 0) return;
    const bool first_step = a.flags & 1, nesterov = a.flags & 2;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int oi = i0 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        if (oi >= C || !jok) continue;
        const size_t e = (size_t)oi * D + j;
        const float g = acc[r] + red[0][lane][r] + red[1][lane][r] + red[2][lane][r];
        a.gW[e] = g;
        if (a.update) {
            const float d = g + a.wd * p[r];
            const float buf = first_step ? d : a.momentum * mo[r] + d;
            a.mW[e] = buf;
            a.pW[e] = p[r] - a.lr * (nesterov ? d + a.momentum * buf : buf);
        }
    }
    if (blockIdx.x == 0) {                                      // the owners of feature column 0 own the bias
        rsum += rs[0][lane] + rs[1][lane] + rs[2][lane];
        rsum += __shfl_xor(rsum, 32, 64);
        if (lk == 0 && iok) {
            a.gB[i] = rsum;
            if (a.update) {
                const float d = rsum + a.wd * pb0;
                const float buf = first_step ? d : a.momentum * mb0 + d;
                a.mB[i] = buf;
                a.pB[i] = pb0 - a.lr * (nesterov ? d + a.momentum * buf : buf);
            }
        }
    }
}

template <bool STEP, int NS>
int pb_launch_fwd(const ProbeArgs& a, hipStream_t s) {
    if (reserve_lds<probe_fwd_kernel<STEP, NS>, PB_LDS_MAX>("probe_fwd_kernel")) return -1;
    const size_t lds = ((size_t)PB_ROWS * (a.D + PB_PAD) + 2 * (size_t)a.D) * 4;
    hipLaunchKernelGGL((probe_fwd_kernel<STEP, NS>), dim3(ceil_div(a.B, PB_ROWS)), dim3(PB_THREADS), lds, s, a);
    LAUNCH_OK("probe_fwd_kernel");
    return 0;
}

}  // namespace

// the limits of the kernels, checked on the host before any launch
int pevit_probe_check(int D, int C, const char* who) {
    if (D < 16 || D > PB_MAX_D || D % 16) {
        pevit_set_error("%s: feature width %d must be a multiple of 16 in [16, %d]", who, D, PB_MAX_D); return -1;
    }
    if (C < 1 || C > PB_MAX_C) { pevit_set_error("%s: %d classes outside [1, %d]", who, C, PB_MAX_C); return -1; }
    return 0;
}

int pevit_launch_probe_step(const ProbeArgs& a, hipStream_t s) {
    if (pevit_probe_check(a.D, a.C, "probe_step")) return -1;
    if (a.B < 2) { pevit_set_error("probe_step: batch %d must be at least 2", a.B); return -1; }
    int rc;
    if (a.C <= 128) rc = pb_launch_fwd<true, 2>(a, s);
    else if (a.C <= 256) rc = pb_launch_fwd<true, 4>(a, s);
    else if (a.C <= 512) rc = pb_launch_fwd<true, 8>(a, s);
    else rc = pb_launch_fwd<true, 16>(a, s);
    if (rc) return rc;
    hipLaunchKernelGGL(probe_update_kernel, dim3(ceil_div(a.D, 32), ceil_div(a.C, 32)), dim3(PB_THREADS), 0, s, a);
    LAUNCH_OK("probe_update_kernel");
    return 0;
}

int pevit_launch_probe_predict(const ProbeArgs& a, hipStream_t s) {
    if (pevit_probe_check(a.D, a.C, "probe_predict")) return -1;
    if (a.B < 1) { pevit_set_error("probe_predict: %d rows (at least 1)", a.B); return -1; }
    return pb_launch_fwd<false, 2>(a, s);
}
