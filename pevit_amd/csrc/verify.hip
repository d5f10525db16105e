// f32-class VERIFICATION kernels (weight_format PEVIT_W_F32_VERIFY).
//
// BASELINE.md states the bf16 gates (logits <= 2e-2, gradients <= 5e-2 rel-L2) for parity with the reference.  On the
// randomly initialised, 12-24 layer towers of the fixtures, bf16 OPERAND ROUNDING ALONE moves logits by 3-10 % and
// individual gradients by up to 50 % (the f32 oracle with nothing changed but its contraction operands rounded to bf16
// shows the same spread, tests/test_gpu_tower.py) -- chaotic amplification, not a kernel property, and no
// bf16-operand engine can meet the stated gates on those inputs.  This mode separates "rounding" from "bug": the SAME
// launch sequences, memory layouts, index arithmetic (raw-reshape scramble, head layout, class-token pruning, chain
// rules, flat parameter buffer) and f32 kernels (LayerNorm, head, optimizer, chain rules) run with every activation and
// weight kept in f32, and the matrix-core contractions replaced by the plain f32 kernels of this file.  In this mode the
// stated gates are asserted against the reference's fixtures as written (tests/test_gpu_verify.py).  It is a test mode:
// ~20x slower, never benchmarked.
//
// Kernels: naive tiled f32 GEMM with the production epilogues (gemm_epilogue.h), attention forward / backward with f32
// softmax statistics, and the token-contracted low-rank adapter products.  All sums run in a fixed order (deterministic).
#include "common.h"
#include "kernels.h"
#include "mfma_frag.h"
#include "gemm_epilogue.h"
#include "../../include/pevit_hip.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// C[M,N] = A[M,K] B[N,K]^T, f32 operands.  64x64 tile, 256 threads, thread = 2 rows x 8 columns.
template <int EPI>
__global__ __launch_bounds__(256) void gemm_f32_kernel(GemmParams p) {
    constexpr int BK = 32;
    __shared__ float As[64][BK + 1];
    __shared__ float Bs[64][BK + 1];
    const float* A = reinterpret_cast<const float*>(p.A);
    const float* B = reinterpret_cast<const float*>(p.B);
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int t = threadIdx.x, r0 = (t >> 3) * 2, c0 = (t & 7) * 8;
    float acc[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
    for (int k0 = 0; k0 < p.K; k0 += BK) {
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int idx = t + 256 * it, r = idx >> 5, k = idx & 31;
            int ar = m0 + r; ar = ar < p.M ? ar : p.M - 1;
            int br = n0 + r; br = br < p.Nb ? br : p.Nb - 1;
            As[r][k] = A[(size_t)ar * p.lda + k0 + k];
            Bs[r][k] = B[(size_t)br * p.ldb + k0 + k];
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < BK; ++k) {
            const float a0 = As[r0][k], a1 = As[r0 + 1][k];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float b = Bs[c0 + j][k];
                acc[0][j] = fmaf(a0, b, acc[0][j]);
                acc[1][j] = fmaf(a1, b, acc[1][j]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = m0 + r0 + i, col = n0 + c0;
        if (row < p.M && col < p.N) epilogue_store<EPI, float>(p, row, col, acc[i]);
    }
}

template <int EPI>
int launch_f32(const GemmParams& p, hipStream_t s) {
    hipLaunchKernelGGL(gemm_f32_kernel<EPI>, dim3(ceil_div(p.N, 64), ceil_div(p.M, 64)), dim3(256), 0, s, p);
    LAUNCH_OK("gemm_f32_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// attention, one (batch, head) per workgroup, q/k/v (B*H, N, 64) f32, out / dout rows (b*N+n), cols h*64+d
__global__ __launch_bounds__(256) void attn_fwd_f32_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                           const float* __restrict__ v, float* __restrict__ out, int ldo,
                                                           float* __restrict__ lse, int H, int N) {
    const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
    const float* kh = k + (size_t)bh * N * 64;
    const float* vh = v + (size_t)bh * N * 64;
    for (int i = threadIdx.x; i < N; i += 256) {
        float qi[64];
#pragma unroll
        for (int d = 0; d < 64; ++d) qi[d] = q[((size_t)bh * N + i) * 64 + d];
        float m = -3.0e38f;
        for (int j = 0; j < N; ++j) {
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < 64; ++d) s = fmaf(qi[d], kh[(size_t)j * 64 + d], s);
            m = fmaxf(m, s);
        }
        float l = 0.f, o[64];
#pragma unroll
        for (int d = 0; d < 64; ++d) o[d] = 0.f;
        for (int j = 0; j < N; ++j) {
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < 64; ++d) s = fmaf(qi[d], kh[(size_t)j * 64 + d], s);
            const float pj = expf(s - m);
            l += pj;
#pragma unroll
            for (int d = 0; d < 64; ++d) o[d] = fmaf(pj, vh[(size_t)j * 64 + d], o[d]);
        }
        const float inv = 1.0f / l;
        float* dst = out + ((size_t)b * N + i) * ldo + h * 64;
#pragma unroll
        for (int d = 0; d < 64; ++d) dst[d] = o[d] * inv;
        lse[(size_t)bh * N + i] = m + logf(l);
    }
}

// attention probabilities (attn_probs.hip) in f32: one thread per (image, query, key), S = q . k over d = 64, P = exp(S - lse),
// summed over the heads in order and divided by H (average), or stored per head
__global__ __launch_bounds__(256) void attn_probs_f32_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                             const float* __restrict__ lse, float* __restrict__ out, int B, int H, int N,
                                                             int average) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)B * N * N) return;
    const int col = (int)(idx % N), row = (int)((idx / N) % N), b = (int)(idx / ((size_t)N * N));
    float sum = 0.f;
    for (int h = 0; h < H; ++h) {
        const size_t bh = (size_t)b * H + h;
        const float* qi = q + (bh * N + row) * 64;
        const float* kj = k + (bh * N + col) * 64;
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < 64; ++d) s = fmaf(qi[d], kj[d], s);
        const float p = expf(s - lse[bh * N + row]);
        if (average) sum += p;
        else out[(bh * N + row) * N + col] = p;
    }
    if (average) out[idx] = sum / (float)H;
}

__global__ __launch_bounds__(256) void attn_bwd_f32_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                           const float* __restrict__ v, const float* __restrict__ out, int ldo,
                                                           const float* __restrict__ dout, int lddo,
                                                           const float* __restrict__ lse, float* __restrict__ dqkv, int ld,
                                                           int H, int N) {
    __shared__ float del[320];
    const int bh = blockIdx.x, b = bh / H, h = bh - b * H, E = H * 64;
    const float* qh = q + (size_t)bh * N * 64;
    const float* kh = k + (size_t)bh * N * 64;
    const float* vh = v + (size_t)bh * N * 64;
    const float* oh = out + (size_t)b * N * ldo + h * 64;
    const float* doh = dout + (size_t)b * N * lddo + h * 64;
    const float* lh = lse + (size_t)bh * N;
    for (int i = threadIdx.x; i < N; i += 256) {
        float s = 0.f;
        for (int d = 0; d < 64; ++d) s = fmaf(doh[(size_t)i * lddo + d], oh[(size_t)i * ldo + d], s);
        del[i] = s;
    }
    __syncthreads();
    // dQ_i = sum_j p_ij (dP_ij - delta_i) k_j
    for (int i = threadIdx.x; i < N; i += 256) {
        float qi[64], doi[64], acc[64];
#pragma unroll
        for (int d = 0; d < 64; ++d) { qi[d] = qh[(size_t)i * 64 + d]; doi[d] = doh[(size_t)i * lddo + d]; acc[d] = 0.f; }
        const float li = lh[i], di = del[i];
        for (int j = 0; j < N; ++j) {
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < 64; ++d) { s = fmaf(qi[d], kh[(size_t)j * 64 + d], s); dp = fmaf(doi[d], vh[(size_t)j * 64 + d], dp); }
            const float ds = expf(s - li) * (dp - di);
#pragma unroll
            for (int d = 0; d < 64; ++d) acc[d] = fmaf(ds, kh[(size_t)j * 64 + d], acc[d]);
        }
        float* dst = dqkv + ((size_t)b * N + i) * ld + h * 64;
#pragma unroll
        for (int d = 0; d < 64; ++d) dst[d] = acc[d];
    }
    // dK_j = sum_i ds_ij q_i ; dV_j = sum_i p_ij dO_i
    for (int j = threadIdx.x; j < N; j += 256) {
        float kj[64], vj[64], ak[64], av[64];
#pragma unroll
        for (int d = 0; d < 64; ++d) { kj[d] = kh[(size_t)j * 64 + d]; vj[d] = vh[(size_t)j * 64 + d]; ak[d] = 0.f; av[d] = 0.f; }
        for (int i = 0; i < N; ++i) {
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < 64; ++d) { s = fmaf(qh[(size_t)i * 64 + d], kj[d], s); dp = fmaf(doh[(size_t)i * lddo + d], vj[d], dp); }
            const float pij = expf(s - lh[i]);
            const float ds = pij * (dp - del[i]);
#pragma unroll
            for (int d = 0; d < 64; ++d) {
                ak[d] = fmaf(ds, qh[(size_t)i * 64 + d], ak[d]);
                av[d] = fmaf(pij, doh[(size_t)i * lddo + d], av[d]);
            }
        }
        float* dst = dqkv + ((size_t)b * N + j) * ld + h * 64;
#pragma unroll
        for (int d = 0; d < 64; ++d) { dst[E + d] = ak[d]; dst[2 * E + d] = av[d]; }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// low-rank adapter products (lowrank.hip states the math and the flat addressing)

// u[row(rr)][j] = sum_e dDelta_{q|v}[rr][e] Q32[e][j]    thread = (rr, j)
__global__ void lowrank_u_f32_kernel(const float* __restrict__ dqkv, int ld, const float* __restrict__ q32, float* __restrict__ u32,
                                     float* __restrict__ ucols, int B, int H, int N, int E) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int T = B * N;
    if (idx >= T * 64) return;
    const int rr = idx >> 6, j = idx & 63;
    const int col0 = j < 32 ? 0 : 2 * E;
    float s = 0.f;
    for (int e0 = 0; e0 < E; e0 += 64) {
        const float* slab = ddelta_slab(dqkv, ld, col0, rr, e0, E, H, N);
        for (int d = 0; d < 64; ++d) s = fmaf(slab[d], q32[(size_t)(e0 + d) * 64 + j], s);
    }
    const int row = row_of_ref(rr, B, N);
    u32[(size_t)row * 64 + j] = s;
    ucols[(size_t)row * ld + j] = s;
}

// same partial layout as lowrank_grad_kernel: partial[chunk][4][E][32], dbias_partial[chunk][2][E]
constexpr int VG_ROWS = 256;       // == LG_ROWS of lowrank.hip (pevit_lowrank_chunks)
__global__ __launch_bounds__(256) void lowrank_grad_f32_kernel(const float* __restrict__ xn, int ldx, const float* __restrict__ u32,
                                                               const float* __restrict__ dqkv, int ld, const float* __restrict__ t,
                                                               float* __restrict__ partial, float* __restrict__ dbias_partial,
                                                               int B, int H, int N, int E) {
    const int epairs = E / 64, per_chunk = epairs * 3;
    const int chunk = blockIdx.x / per_chunk, rem = blockIdx.x - chunk * per_chunk;
    const int kind = rem / epairs, e0 = (rem - kind * epairs) * 64;
    const int T = B * N, r0 = chunk * VG_ROWS, r1 = min(T, r0 + VG_ROWS);
    const size_t plane = (size_t)E * 32;
    const int tid = threadIdx.x;
    if (kind == 0) {        // G0/G1[e][j] = sum_r xn[r][e] u[r][j | 32+j]
        for (int o = tid; o < 64 * 64; o += 256) {
            const int e = e0 + (o >> 6), jj = o & 63;
            float s = 0.f;
            for (int r = r0; r < r1; ++r) s = fmaf(xn[(size_t)r * ldx + e], u32[(size_t)r * 64 + jj], s);
            partial[((size_t)chunk * 4 + (jj >> 5)) * plane + (size_t)e * 32 + (jj & 31)] = s;
        }
    } else {                // G2/G3[e][j] = sum_rr dDelta[rr][e] t[row(rr)][j (+32)] ; d bias = column sums of dDelta
        const int col0 = kind == 1 ? 0 : 2 * E, toff = kind == 1 ? 0 : 32;
        for (int o = tid; o < 64 * 32; o += 256) {
            const int d = o >> 5, j = o & 31;
            float s = 0.f;
            for (int rr = r0; rr < r1; ++rr)
                s = fmaf(ddelta_slab(dqkv, ld, col0, rr, e0, E, H, N)[d], t[(size_t)row_of_ref(rr, B, N) * 64 + toff + j], s);
            partial[((size_t)chunk * 4 + kind + 1) * plane + (size_t)(e0 + d) * 32 + j] = s;
        }
        if (tid < 64) {
            float s = 0.f;
            for (int rr = r0; rr < r1; ++rr) s += ddelta_slab(dqkv, ld, col0, rr, e0, E, H, N)[tid];
            dbias_partial[((size_t)chunk * 2 + (kind - 1)) * E + e0 + tid] = s;
        }
    }
}

// post-MLP adapters: partial[chunk][E][64], csx[chunk][E], csy[chunk][64] exactly as tn_gemm64_kernel writes them
constexpr int VT_ROWS = 256;       // == TG_ROWS of adapter.hip (pevit_tn_chunks)
__global__ __launch_bounds__(256) void tn_gemm64_f32_kernel(const float* __restrict__ X, int ldx, const float* __restrict__ Y, int ldy,
                                                            float* __restrict__ partial, float* __restrict__ csx,
                                                            float* __restrict__ csy, int T, int E) {
    const int eslabs = E / 64;
    const int chunk = blockIdx.x / eslabs, e0 = (blockIdx.x - chunk * eslabs) * 64;
    const int r0 = chunk * VT_ROWS, r1 = min(T, r0 + VT_ROWS), tid = threadIdx.x;
    for (int o = tid; o < 64 * 64; o += 256) {
        const int e = e0 + (o >> 6), j = o & 63;
        float s = 0.f;
        for (int r = r0; r < r1; ++r) s = fmaf(X[(size_t)r * ldx + e], Y[(size_t)r * ldy + j], s);
        partial[(size_t)chunk * E * 64 + (size_t)e * 64 + j] = s;
    }
    if (tid < 64) {
        if (csx) { float s = 0.f; for (int r = r0; r < r1; ++r) s += X[(size_t)r * ldx + e0 + tid]; csx[(size_t)chunk * E + e0 + tid] = s; }
        if (csy && e0 == 0) { float s = 0.f; for (int r = r0; r < r1; ++r) s += Y[(size_t)r * ldy + tid]; csy[(size_t)chunk * 64 + tid] = s; }
    }
}

// the f32 twins take their production sibling's parameter struct: its bf16-declared members hold f32 in this mode
inline const float* f32p(const bf16* p) { return reinterpret_cast<const float*>(p); }
inline float* f32p(bf16* p) { return reinterpret_cast<float*>(p); }

}  // namespace

int pevit_launch_tn_gemm64_f32(const TnGemm64Args& a, hipStream_t s) {
    if (a.E % 64) { pevit_set_error("tn_gemm64 (f32 verification): bad width %d", a.E); return -1; }
    hipLaunchKernelGGL(tn_gemm64_f32_kernel, dim3(ceil_div(a.T, VT_ROWS) * (a.E / 64)), dim3(256), 0, s, f32p(a.X), a.ldx, f32p(a.Y), a.ldy, a.partial,
                       a.csx, a.csy, a.T, a.E);
    LAUNCH_OK("tn_gemm64_f32_kernel");
    return 0;
}

int pevit_launch_gemm_f32(int epi, const GemmParams& p, hipStream_t s) {
    if (p.M <= 0 || p.N <= 0 || p.K <= 0 || p.K % 32 || p.N % 8) {
        pevit_set_error("gemm (f32 verification): bad problem M=%d N=%d K=%d", p.M, p.N, p.K); return -1;
    }
    switch (epi) {
        case EPI_QKV_HEADS: return launch_f32<EPI_QKV_HEADS>(p, s);
        case EPI_BIAS_RESID_F32: return launch_f32<EPI_BIAS_RESID_F32>(p, s);
        case EPI_BIAS_GELU: return launch_f32<EPI_BIAS_GELU>(p, s);
        case EPI_DGELU_BF16: return launch_f32<EPI_DGELU_BF16>(p, s);
        case EPI_F32: return launch_f32<EPI_F32>(p, s);
        case EPI_BF16: return launch_f32<EPI_BF16>(p, s);
        case EPI_BIAS_BF16: return launch_f32<EPI_BIAS_BF16>(p, s);
        case EPI_PATCH_EMBED: return launch_f32<EPI_PATCH_EMBED>(p, s);
        case EPI_BIAS_RELU_BF16: return launch_f32<EPI_BIAS_RELU_BF16>(p, s);
        case EPI_BIAS_RESID_KEEP: return launch_f32<EPI_BIAS_RESID_KEEP>(p, s);
        case EPI_BIAS_GELUNEW: return launch_f32<EPI_BIAS_GELUNEW>(p, s);
        case EPI_DRELU_BF16: return launch_f32<EPI_DRELU_BF16>(p, s);
        case EPI_DGELUNEW_BF16: return launch_f32<EPI_DGELUNEW_BF16>(p, s);
        case EPI_BIAS_F32: return launch_f32<EPI_BIAS_F32>(p, s);
        case EPI_BIAS_GELU_ONLY: return launch_f32<EPI_BIAS_GELU_ONLY>(p, s);
    }
    pevit_set_error("gemm (f32 verification): unknown epilogue %d", epi);
    return -1;
}

int pevit_launch_attn_fwd_f32(const AttnArgs& a, hipStream_t s) {
    if (a.N < 1 || a.N > 320) { pevit_set_error("attn_fwd (f32 verification): N=%d outside [1,320]", a.N); return -1; }
    hipLaunchKernelGGL(attn_fwd_f32_kernel, dim3(a.B * a.H), dim3(256), 0, s, f32p(a.q), f32p(a.k), f32p(a.v), f32p(a.out), a.ldo, a.lse, a.H, a.N);
    LAUNCH_OK("attn_fwd_f32_kernel");
    return 0;
}

namespace {
// causal attention of the text tower (attn_causal.hip) in f32: attn_fwd_f32_kernel with query i bounded to the keys j <= i, no lse
__global__ __launch_bounds__(128) void attn_fwd_causal_f32_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                  const float* __restrict__ v, float* __restrict__ out, int ldo,
                                                                  int H, int N) {
    const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
    const float* kh = k + (size_t)bh * N * 64;
    const float* vh = v + (size_t)bh * N * 64;
    for (int i = threadIdx.x; i < N; i += 128) {
        float qi[64];
#pragma unroll
        for (int d = 0; d < 64; ++d) qi[d] = q[((size_t)bh * N + i) * 64 + d];
        float m = -3.0e38f;
        for (int j = 0; j <= i; ++j) {
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < 64; ++d) s = fmaf(qi[d], kh[(size_t)j * 64 + d], s);
            m = fmaxf(m, s);
        }
        float l = 0.f, o[64];
#pragma unroll
        for (int d = 0; d < 64; ++d) o[d] = 0.f;
        for (int j = 0; j <= i; ++j) {
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < 64; ++d) s = fmaf(qi[d], kh[(size_t)j * 64 + d], s);
            const float pj = expf(s - m);
            l += pj;
#pragma unroll
            for (int d = 0; d < 64; ++d) o[d] = fmaf(pj, vh[(size_t)j * 64 + d], o[d]);
        }
        const float inv = 1.0f / l;
        float* dst = out + ((size_t)b * N + i) * ldo + h * 64;
#pragma unroll
        for (int d = 0; d < 64; ++d) dst[d] = o[d] * inv;
    }
}
}  // namespace

int pevit_launch_attn_fwd_causal_f32(const AttnArgs& a, hipStream_t s) {
    if (a.N < 1 || a.N > 128) { pevit_set_error("attn_fwd_causal (f32 verification): N=%d outside [1,128]", a.N); return -1; }
    hipLaunchKernelGGL(attn_fwd_causal_f32_kernel, dim3(a.B * a.H), dim3(128), 0, s, f32p(a.q), f32p(a.k), f32p(a.v), f32p(a.out), a.ldo, a.H, a.N);
    LAUNCH_OK("attn_fwd_causal_f32_kernel");
    return 0;
}

int pevit_launch_attn_bwd_f32(const AttnArgs& a, hipStream_t s) {
    if (a.N < 1 || a.N > 320) { pevit_set_error("attn_bwd (f32 verification): N=%d outside [1,320]", a.N); return -1; }
    hipLaunchKernelGGL(attn_bwd_f32_kernel, dim3(a.B * a.H), dim3(256), 0, s, f32p(a.q), f32p(a.k), f32p(a.v), f32p(a.out), a.ldo, f32p(a.dout), a.lddo,
                       a.lse, f32p(a.dqkv), a.ld, a.H, a.N);
    LAUNCH_OK("attn_bwd_f32_kernel");
    return 0;
}

int pevit_launch_attn_probs_f32(const AttnArgs& a, hipStream_t s) {
    if (a.N < 1 || a.N > 384) { pevit_set_error("attn_probs (f32 verification): N=%d outside [1,384]", a.N); return -1; }
    const size_t n = (size_t)a.B * a.N * a.N;
    hipLaunchKernelGGL(attn_probs_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, f32p(a.q), f32p(a.k), a.lse, a.probs, a.B, a.H, a.N,
                       a.average);
    LAUNCH_OK("attn_probs_f32_kernel");
    return 0;
}

int pevit_launch_lowrank_u_f32(const LowrankArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(lowrank_u_f32_kernel, dim3(ceil_div(a.B * a.N * 64, 256)), dim3(256), 0, s, f32p(a.dqkv), a.ld, a.q32, a.u32, f32p(a.u_bf16_cols),
                       a.B, a.H, a.N, a.E);
    LAUNCH_OK("lowrank_u_f32_kernel");
    return 0;
}

int pevit_launch_lowrank_grad_f32(const LowrankArgs& a, hipStream_t s) {
    if (a.chunks != ceil_div(a.B * a.N, VG_ROWS)) { pevit_set_error("lowrank_grad (f32 verification): chunks mismatch"); return -1; }
    hipLaunchKernelGGL(lowrank_grad_f32_kernel, dim3(a.chunks * (a.E / 64) * 3), dim3(256), 0, s, f32p(a.xn), a.ldx, a.u32, f32p(a.dqkv), a.ld, a.t,
                       a.partial, a.dbias_partial, a.B, a.H, a.N, a.E);
    LAUNCH_OK("lowrank_grad_f32_kernel");
    return 0;
}

// ===============================================================================================================
// TEST-ONLY C-ABI ENTRY POINTS (pevit_op_*_ex).  They hold no kernel: each fills the parameter struct of an existing production
// launcher by name and calls it, so that the forms that only the training step selects -- strided class-token rows, the in-place
// bf16 residual gradient, the power-of-two column scales, the e4m3 copies, the class-token-only dO -- can be launched one kernel
// at a time (tests/test_gpu_kernel_forms.py).  They live in this file because it holds nothing of the profiled production step.
extern "C" int pevit_op_ln_fwd_ex(void* stream, const float* x, const float* gamma, const float* beta, int rows, int E, size_t xstride,
                                  void* y_bf16, float* y_f32, float* mean, float* rstd, void* y_fp8) {
    LnFwdArgs a;
    a.x = x; a.gamma = gamma; a.beta = beta; a.rows = rows; a.E = E; a.xstride = xstride;
    a.y_bf16 = (bf16*)y_bf16; a.y_f32 = y_f32; a.mean = mean; a.rstd = rstd; a.y_fp8 = (unsigned char*)y_fp8;
    return pevit_launch_ln_fwd(a, (hipStream_t)stream);
}
// dy: f32, or (dy_stored) bf16.  dres: f32, or (res16) bf16 -- it may then be dx_bf16 itself, and dx may be null.
extern "C" int pevit_op_ln_bwd_ex(void* stream, const void* dy, int dy_stored, const float* x, const float* mean, const float* rstd,
                                  const float* gamma, const void* dres, int res16, int res_period, float* dx, void* dx_bf16,
                                  int rows, int E, size_t xstride, const float* bf16_colscale, const float* res_colscale) {
    LnBwdArgs a;
    a.dy = dy; a.dy_stored = dy_stored; a.x = x; a.mean = mean; a.rstd = rstd; a.gamma = gamma;
    a.dres = (const float*)dres; a.res16 = res16; a.res_period = res_period; a.dx_out = dx; a.dx_bf16 = (bf16*)dx_bf16;
    a.rows = rows; a.E = E; a.xstride = xstride; a.bf16_colscale = bf16_colscale; a.res_colscale = res_colscale;
    return pevit_launch_ln_bwd(a, (hipStream_t)stream);
}
// out_fp8: e4m3 copy of out (k-permuted, row pitch ldo codes), or null
extern "C" int pevit_op_attn_fwd_ex(void* stream, const void* q, const void* k, const void* v, void* out, int ldo, float* lse,
                                    int B, int H, int N, void* out_fp8) {
    AttnArgs a;
    a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v; a.out = (bf16*)out; a.ldo = ldo; a.lse = lse; a.B = B; a.H = H; a.N = N;
    a.out_fp8 = (unsigned char*)out_fp8;
    return pevit_launch_attn_fwd(a, (hipStream_t)stream);
}
extern "C" int pevit_op_attn_bwd_ex(void* stream, const void* q, const void* k, const void* v, const void* out, int ldo,
                                    const void* dout, int lddo, const float* lse, void* dqkv, int ld, int B, int H, int N,
                                    int dout_cls_only) {
    AttnArgs a;      // (out and lse are only read by the backward)
    a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v; a.out = (bf16*)const_cast<void*>(out); a.ldo = ldo;
    a.lse = const_cast<float*>(lse); a.B = B; a.H = H; a.N = N; a.dout = (const bf16*)dout; a.lddo = lddo; a.dqkv = (bf16*)dqkv; a.ld = ld;
    a.dout_cls_only = dout_cls_only;
    return pevit_launch_attn_bwd(a, (hipStream_t)stream);
}
// The fused post-MLP adapter launches (adapter_fused.hip; tests/test_gpu_adapter_fused.py): every member of AdapterFwdArgs /
// AdapterBwdArgs by name, the contraction range of the backward included.
extern "C" int pevit_op_adapter_fwd_ex(void* stream, const pevit_adapter_fwd_args* a) {
    if (!a) { pevit_set_error("adapter_fwd_ex: null argument struct"); return -1; }
    AdapterFwdArgs p;
    p.act_kind = a->act_kind; p.T = a->T; p.E = a->E;
    p.hraw = a->hraw; p.bpr = a->bpr; p.x_mid = a->x_mid; p.gamma = a->gamma; p.beta = a->beta;
    p.wd = (const bf16*)a->wd; p.b_down = a->b_down; p.wu = (const bf16*)a->wu; p.b_up = a->b_up;
    p.z = (bf16*)a->z; p.mean_a = a->mean_a; p.rstd_a = a->rstd_a; p.act = (bf16*)a->act; p.apre = (bf16*)a->apre; p.x_out = a->x_out;
    return pevit_launch_adapter_fwd(p, (hipStream_t)stream);
}
extern "C" int pevit_op_adapter_bwd_ex(void* stream, const pevit_adapter_bwd_args* a) {
    if (!a) { pevit_set_error("adapter_bwd_ex: null argument struct"); return -1; }
    AdapterBwdArgs p;
    p.act_kind = a->act_kind; p.T = a->T; p.E = a->E;
    p.dyb = (const bf16*)a->dyb; p.dres = a->dres; p.wuT = (const bf16*)a->wuT; p.saved = (const bf16*)a->saved; p.wdT = (const bf16*)a->wdT;
    p.hraw = a->hraw; p.bpr = a->bpr; p.mean_a = a->mean_a; p.rstd_a = a->rstd_a; p.gamma = a->gamma;
    p.dpre = (bf16*)a->dpre; p.dh_bf16 = (bf16*)a->dh_bf16; p.partial = a->partial;
    p.tn_x1 = (const bf16*)a->tn_x1; p.tn_y1 = (const bf16*)a->tn_y1; p.tn_partial1 = a->tn_partial1;
    p.tn_x2 = (const bf16*)a->tn_x2; p.tn_y2 = (const bf16*)a->tn_y2; p.tn_partial2 = a->tn_partial2; p.tn_csy2 = a->tn_csy2;
    p.tn_blocks = a->tn_blocks;
    return pevit_launch_adapter_bwd(p, (hipStream_t)stream);
}
// The attention-site low-rank adapter launches (lowrank.hip and its f32 twins above; tests/test_gpu_lowrank.py): every member of
// LowrankArgs, PrepKadaptArgs / PrepLoraArgs and ChainKadaptArgs / ChainLoraArgs by name.
extern "C" int pevit_op_lowrank_ex(void* stream, const pevit_lowrank_args* a) {
    if (!a) { pevit_set_error("lowrank_ex: null argument struct"); return -1; }
    LowrankArgs p;
    p.dqkv = (const bf16*)a->dqkv; p.ld = a->ld; p.qT = (const bf16*)a->qT; p.q32 = a->q32; p.u32 = a->u32; p.u_bf16_cols = (bf16*)a->u_bf16_cols;
    p.xn = (const bf16*)a->xn; p.ldx = a->ldx; p.t = a->t; p.partial = a->partial; p.dbias_partial = a->dbias_partial; p.chunks = a->chunks;
    p.B = a->B; p.H = a->H; p.N = a->N; p.E = a->E; p.xcd_order = a->xcd_order; p.this_layer = a->this_layer; p.prev = a->prev;
    p.xn_prev = (const bf16*)a->xn_prev; p.u32_prev = a->u32_prev; p.partial_prev = a->partial_prev;
    if (p.B < 1 || p.N < 1 || p.H < 1) { pevit_set_error("lowrank_ex: B=%d H=%d N=%d", p.B, p.H, p.N); return -1; }
    hipStream_t s = (hipStream_t)stream;
    switch (a->form) {
        case PEVIT_LOWRANK_U: return pevit_launch_lowrank_u(p, s);
        case PEVIT_LOWRANK_GRAD: return pevit_launch_lowrank_grad(p, s);
        case PEVIT_LOWRANK_COMBO: return pevit_launch_lowrank_combo(p, s);
        case PEVIT_LOWRANK_U_F32: return pevit_launch_lowrank_u_f32(p, s);
        case PEVIT_LOWRANK_GRAD_F32: return pevit_launch_lowrank_grad_f32(p, s);
    }
    pevit_set_error("lowrank_ex: unknown form %d", a->form);
    return -1;
}
extern "C" int pevit_op_prep_lowrank(void* stream, const pevit_prep_lowrank_args* a) {
    if (!a) { pevit_set_error("prep_lowrank: null argument struct"); return -1; }
    AdapterPanels pan;
    pan.w_aug_rows = (bf16*)a->w_aug_rows; pan.ldw = a->ldw; pan.wT_aug_cols = (bf16*)a->wT_aug_cols; pan.ldwT = a->ldwT;
    pan.q32 = a->q32; pan.qT = (bf16*)a->qT; pan.q16 = (bf16*)a->q16;
    LayerStrides st;
    st.arena_bytes = a->arena_bytes; st.param_floats = a->param_floats;
    if (a->method == PEVIT_KADAPTATION) {
        PrepKadaptArgs p;
        p.rule1_l = a->rule1_l; p.rule1_r = a->rule1_r; p.rule2_l = a->rule2_l; p.rule2_r = a->rule2_r; p.q_left = a->q_left; p.q_right = a->q_right;
        p.pan = pan; p.E = a->E; p.ascale = a->ascale; p.layers = a->layers; p.st = st; p.f32 = a->f32;
        return pevit_launch_prep_kadapt(p, (hipStream_t)stream);
    }
    if (a->method == PEVIT_LORA) {
        PrepLoraArgs p;
        p.a1q = a->a1q; p.a2q = a->a2q; p.a1v = a->a1v; p.a2v = a->a2v; p.r = a->r;
        p.pan = pan; p.E = a->E; p.ascale = a->ascale; p.layers = a->layers; p.st = st; p.f32 = a->f32;
        return pevit_launch_prep_lora(p, (hipStream_t)stream);
    }
    pevit_set_error("prep_lowrank: method %d has no attention-site panels", a->method);
    return -1;
}
extern "C" int pevit_op_chain_lowrank(void* stream, const pevit_chain_lowrank_args* a) {
    if (!a) { pevit_set_error("chain_lowrank: null argument struct"); return -1; }
    if (a->method == PEVIT_KADAPTATION) {
        ChainKadaptArgs p;
        p.partial = a->partial; p.partial_layer = a->partial_layer; p.dbias_partial = a->dbias_partial; p.dbias_layer = a->dbias_layer;
        p.chunks = a->chunks; p.ascale = a->ascale; p.layers = a->layers; p.G = a->G; p.rule_scratch = a->rule_scratch;
        p.params = a->params; p.grads = a->grads; p.p_layer0 = a->p_layer0; p.p_layer_stride = a->p_layer_stride; p.E = a->E;
        return pevit_launch_chain_kadapt(p, (hipStream_t)stream);
    }
    if (a->method == PEVIT_LORA) {
        ChainLoraArgs p;
        p.partial = a->partial; p.partial_layer = a->partial_layer; p.chunks = a->chunks; p.ascale = a->ascale; p.r = a->r; p.layers = a->layers;
        p.G = a->G; p.grads = a->grads; p.p_layer0 = a->p_layer0; p.p_layer_stride = a->p_layer_stride; p.E = a->E;
        return pevit_launch_chain_lora(p, (hipStream_t)stream);
    }
    pevit_set_error("chain_lowrank: method %d has no attention-site chain rule", a->method);
    return -1;
}
extern "C" int pevit_op_rule_sum(void* stream, const float* rule_scratch, float* grads, int l_lo, int l_hi) {
    return pevit_launch_rule_sum(rule_scratch, grads, l_lo, l_hi, (hipStream_t)stream);
}
extern "C" int pevit_op_lowrank_plan(int B, int N, int E, int this_layer, int prev, int32_t out[5]) {
    if (!out || B < 1 || N < 1 || E < 64 || E % 64) { pevit_set_error("lowrank_plan: B=%d N=%d E=%d", B, N, E); return -1; }
    const int combo = this_layer || prev;
    const LowrankPlan p = pevit_lowrank_plan(B, N, E, combo, this_layer, prev);
    if (!p.es) { pevit_set_error("lowrank_plan: no slab grouping for width %d", E); return -1; }
    out[0] = p.es; out[1] = p.nu; out[2] = p.n12; out[3] = p.n0; out[4] = p.chunks;
    return 0;
}
// The classifier head (stem_head.hip; tests/test_gpu_head.py): every member of HeadArgs by name, all scratch the caller's.  What the
// engine's own callers guarantee by construction is refused here, before the first launch.
extern "C" int pevit_op_head_ex(void* stream, const pevit_head_args* a) {
    if (!a) { pevit_set_error("head_ex: null argument struct"); return -1; }
    if (a->B < 1 || a->D < 1 || a->Cc < 1) { pevit_set_error("head_ex: B=%d D=%d C=%d", a->B, a->D, a->Cc); return -1; }
    if (a->labels && a->targets) { pevit_set_error("head_ex: labels and targets are both set"); return -1; }
    if (a->training && a->B < 2) { pevit_set_error("head_ex: training-mode BatchNorm needs B >= 2 (B=%d)", a->B); return -1; }
    if (!a->feat || !a->W || !a->running_mean || !a->running_var || !a->ybn || !a->rstd || !a->logits) {
        pevit_set_error("head_ex: feat, W, running_mean, running_var, ybn, rstd and logits are required"); return -1;
    }
    if ((a->labels || a->targets) && (!a->dlogits || !a->dybn || !a->loss)) {
        pevit_set_error("head_ex: a loss needs dlogits, dybn and loss"); return -1;
    }
    HeadArgs p;
    p.feat = a->feat; p.labels = a->labels; p.targets = a->targets; p.W = a->W; p.bias = a->bias; p.gW = a->gW; p.gb = a->gb;
    p.running_mean = a->running_mean; p.running_var = a->running_var; p.training = a->training;
    p.ybn = a->ybn; p.rstd = a->rstd; p.logits = a->logits; p.dlogits = a->dlogits; p.dybn = a->dybn; p.loss = a->loss;
    p.dfeat = a->dfeat; p.dfeat_bf16 = (bf16*)a->dfeat_bf16; p.B = a->B; p.D = a->D; p.Cc = a->Cc;
    return pevit_launch_head(p, (hipStream_t)stream);
}
// The small exact kernels around the towers (stem_head.hip, misc.hip, text.hip; tests/test_gpu_movers.py): the launchers' arguments
// as they stand, the f32 storage flag included.
extern "C" int pevit_op_conv_weight(void* stream, const float* w, void* out, int E, int K, int Kpad, int f32) {
    return pevit_launch_conv_weight(w, (bf16*)out, E, K, Kpad, (hipStream_t)stream, f32);
}
extern "C" int pevit_op_cls_row(void* stream, const float* cls, const float* pos, float* x, int B, int N, int E) {
    return pevit_launch_cls_row(cls, pos, x, B, N, E, (hipStream_t)stream);
}
extern "C" int pevit_op_im2col_ex(void* stream, const void* images, int u8, const float* mean3, const float* std3, void* patches, int B,
                                  int R, int P, int Kpad, int f32) {
    if (!u8) return pevit_launch_im2col((const float*)images, (bf16*)patches, B, R, P, Kpad, (hipStream_t)stream, f32);
    Im2colU8Args a;
    a.img = (const unsigned char*)images; a.mean3 = mean3; a.std3 = std3; a.out = (bf16*)patches; a.B = B; a.R = R; a.P = P; a.Kp = Kpad;
    a.f32 = f32;
    return pevit_launch_im2col_u8(a, (hipStream_t)stream);
}
extern "C" int pevit_op_cast_ex(void* stream, const float* src, void* dst, size_t n, float scale, int f32) {
    return pevit_launch_cast_bf16(src, (bf16*)dst, n, scale, (hipStream_t)stream, f32);
}
extern "C" int pevit_op_transpose(void* stream, const float* src, int rows, int cols, void* dst, int ldd, int scaled_rows, float scale,
                                  int f32) {
    return pevit_launch_transpose_bf16(src, rows, cols, (bf16*)dst, ldd, scaled_rows, scale, (hipStream_t)stream, f32);
}
extern "C" int pevit_op_permute_rows(void* stream, const float* src, float* dst, int N, int B, int E, int to_internal) {
    return pevit_launch_permute_rows(src, dst, N, B, E, to_internal, (hipStream_t)stream);
}
extern "C" int pevit_op_zero(void* stream, void* ptr, size_t bytes) { return pevit_launch_zero(ptr, bytes, (hipStream_t)stream); }
extern "C" int pevit_op_scale_f32(void* stream, float* p, size_t n, float scale) {
    return pevit_launch_scale_f32(p, n, scale, (hipStream_t)stream);
}
extern "C" int pevit_op_text_embed(void* stream, const int64_t* tokens, const float* table, const float* pos, float* x, int S, int N,
                                   int E, int V) {
    TextEmbedArgs a;
    a.tokens = tokens; a.table = table; a.pos = pos; a.x = x; a.S = S; a.N = N; a.E = E; a.V = V;
    return pevit_launch_text_embed(a, (hipStream_t)stream);
}
extern "C" int pevit_op_text_eot_gather(void* stream, const int64_t* tokens, const float* x, float* rows_out, int S, int N, int E) {
    return pevit_launch_text_eot_gather(tokens, x, rows_out, S, N, E, (hipStream_t)stream);
}
extern "C" int pevit_op_adapter_blocks(int T) { return pevit_adapter_blocks(T); }
extern "C" int pevit_op_adapter_fused_ok(int E) { return pevit_adapter_fused_ok(E) ? 1 : 0; }
