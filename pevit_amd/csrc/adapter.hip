// Post-MLP bottleneck adapters: Adapter (adapter_model.py:204-336) and Compacter
// (compacter_model.py:196-308,356-503).
//
//   x <- x + [ h + up(act(down(LN_a(h)))) ]          h = mlp(ln_2(x))
//
// (the reference's Adapter evaluates mlp(ln_2(x)) twice -- adapter_model.py:333 -- with identical
// values; here h is computed once and its gradient is the sum of both uses).
// Adapter : down = Linear(E,64), act = ReLU,      up = Linear(64,E)
// Compacter: down/up = PHMLinear, H = sum_{i<4} kron(rule_i (4x4), Wl_i Wr_i), act = gelu_new; the
//            shared rule (4,4,4) is frozen (its name lacks "compacter": compacter_clip.py:122).
// Both reduce to two dense E x 64 panels, so they share every kernel: the contractions are the MFMA
// GEMM (gemm.hip; epilogues BIAS_RELU / BIAS_GELUNEW / DRELU / DGELUNEW of gemm_epilogue.h), and this file holds
//   * the panel builders (f32 master parameters -> bf16 panels in both orientations, every step),
//   * the token-contracted weight gradients  G = X^T Y  (LDS-transposed panels + bf16 MFMA),
//   * LayerNorm backward with gradients for the trainable affine (adapter_norm_before),
//   * the chain rule from the dense panels back to the reference's parameter tensors.
#include "common.h"
#include "kernels.h"
#include "gemm_epilogue.h"
#include "mfma_frag.h"

namespace {

constexpr int TG_ROWS = 256;
constexpr int TG_LD = 72;           // row stride (elements) of the row-major LDS tiles

// ---------------------------------------------------------------------------------------------
// panels: wd [64][E] (B operand of the down GEMM), wdT [E][64] (d z GEMM), wu [E][64] (up GEMM),
// wuT [64][E] (d act GEMM).  blockIdx.y = layer.
template <typename ST>
__global__ void prep_adapter_kernel(const float* __restrict__ w_down, const float* __restrict__ w_up, BottleneckPanels pan,
                                    int E, LayerStrides st) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 64 * E) return;
    const size_t lo = (size_t)blockIdx.y;
    w_down += lo * st.param_floats; w_up += lo * st.param_floats;
    char* base = reinterpret_cast<char*>(pan.wd) + lo * st.arena_bytes;
    bf16* wd = reinterpret_cast<bf16*>(base);
    bf16* wdT = reinterpret_cast<bf16*>(base + ((char*)pan.wdT - (char*)pan.wd));
    bf16* wu = reinterpret_cast<bf16*>(base + ((char*)pan.wu - (char*)pan.wd));
    bf16* wuT = reinterpret_cast<bf16*>(base + ((char*)pan.wuT - (char*)pan.wd));
    const int j = idx / E, e = idx - j * E;
    const float d = w_down[(size_t)j * E + e];        // (64, E)
    const float u = w_up[(size_t)e * 64 + j];         // (E, 64)
    st_store<ST>(wd, (size_t)j * E + e, d);
    st_store<ST>(wdT, (size_t)e * 64 + j, d);
    st_store<ST>(wu, (size_t)e * 64 + j, u);
    st_store<ST>(wuT, (size_t)j * E + e, u);
}

// Compacter: H_down[a*Fi+k][c*16+p] = sum_i rule[i][a][c] Wl[i][k] Wr[i][p]   (Fi = E/4)
//            H_up  [a*16+k][c*Fi+p] = sum_i rule[i][a][c] Ul[i][k] Ur[i][p]
// effective dense weights: w_down[j][e] = H_down[e][j], w_up[e][j] = H_up[j][e].
template <typename ST>
__global__ void prep_compacter_kernel(const float* __restrict__ rule, const float* __restrict__ dWl,
                                      const float* __restrict__ dWr, const float* __restrict__ uWl,
                                      const float* __restrict__ uWr, BottleneckPanels pan, int E, LayerStrides st) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 64 * E) return;
    const size_t lo = (size_t)blockIdx.y;
    dWl += lo * st.param_floats; dWr += lo * st.param_floats; uWl += lo * st.param_floats; uWr += lo * st.param_floats;
    char* base = reinterpret_cast<char*>(pan.wd) + lo * st.arena_bytes;
    bf16* wd = reinterpret_cast<bf16*>(base);
    bf16* wdT = reinterpret_cast<bf16*>(base + ((char*)pan.wdT - (char*)pan.wd));
    bf16* wu = reinterpret_cast<bf16*>(base + ((char*)pan.wu - (char*)pan.wd));
    bf16* wuT = reinterpret_cast<bf16*>(base + ((char*)pan.wuT - (char*)pan.wd));
    const int Fi = E / 4;
    const int j = idx / E, e = idx - j * E;
    {   // down: e = a*Fi + k, j = c*16 + p
        const int a = e / Fi, k = e - a * Fi, c = j >> 4, p = j & 15;
        float h = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) h += rule[i * 16 + a * 4 + c] * dWl[i * Fi + k] * dWr[i * 16 + p];
        st_store<ST>(wd, (size_t)j * E + e, h);
        st_store<ST>(wdT, (size_t)e * 64 + j, h);
    }
    {   // up: j = a*16 + k, e = c*Fi + p
        const int a = j >> 4, k = j & 15, c = e / Fi, p = e - c * Fi;
        float h = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) h += rule[i * 16 + a * 4 + c] * uWl[i * 16 + k] * uWr[i * Fi + p];
        st_store<ST>(wu, (size_t)e * 64 + j, h);
        st_store<ST>(wuT, (size_t)j * E + e, h);
    }
}

// ---------------------------------------------------------------------------------------------
// G[e][j] = sum_r X[r][e] Y[r][j]   X: bf16 [T][ldx] (64-column slab per workgroup), Y: bf16 [T][ldy]
// (64 columns).  Workgroup = (chunk of TG_ROWS rows, 64 columns e).  Same structure as
// lowrank_grad_kernel: coalesced 16-byte loads, ROW-major LDS images (16-byte writes), both MFMA operands by the
// transposing LDS read.
// partial[chunk][E][64]; optional column sums of X -> csx[chunk][E], of Y -> csy[chunk][64].
__global__ __launch_bounds__(256) void tn_gemm64_kernel(const bf16* __restrict__ X, int ldx, const bf16* __restrict__ Y,
                                                        int ldy, float* __restrict__ partial, float* __restrict__ csx,
                                                        float* __restrict__ csy, int T, int E) {
    __shared__ __attribute__((aligned(16))) bf16 Xs[TG_ROWS * TG_LD];
    __shared__ __attribute__((aligned(16))) bf16 Ys[TG_ROWS * TG_LD];
    __shared__ float cs[2][4][64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, c16 = lane & 15;
    const int eslabs = E / 64;
    const int chunk = blockIdx.x / eslabs, e0 = (blockIdx.x - chunk * eslabs) * 64;
    const int r0 = chunk * TG_ROWS;
    const int c = tid & 7;
    bf16x8 xv[TG_ROWS / 32], yv[TG_ROWS / 32];
#pragma unroll
    for (int it = 0; it < TG_ROWS / 32; ++it) {
        const int r = r0 + (tid >> 3) + 32 * it;
        xv[it] = zero_bf16x8(); yv[it] = zero_bf16x8();
        if (r < T) {
            xv[it] = load_bf16x8(X + (size_t)r * ldx + e0 + 8 * c);
            yv[it] = load_bf16x8(Y + (size_t)r * ldy + 8 * c);
        }
    }
    float sx[8], sy[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { sx[i] = 0.f; sy[i] = 0.f; }
#pragma unroll
    for (int it = 0; it < TG_ROWS / 32; ++it) {
        const int y = (tid >> 3) + 32 * it;
        *reinterpret_cast<bf16x8*>(Xs + y * TG_LD + 8 * c) = xv[it];
        *reinterpret_cast<bf16x8*>(Ys + y * TG_LD + 8 * c) = yv[it];
#pragma unroll
        for (int i = 0; i < 8; ++i) { sx[i] += bf2f(xv[it][i]); sy[i] += bf2f(yv[it][i]); }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float a = rowlane_sum(sx[i]), b = rowlane_sum(sy[i]);
        if ((lane >> 3) == 0) { cs[0][wid][8 * c + i] = a; cs[1][wid][8 * c + i] = b; }
    }
    __syncthreads();
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < TG_ROWS / 32; ++ks) {
        const bf16x8 a = trfrag<TG_LD>(Xs, ks, 16 * wid, lane);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
            acc[nt] = mfma16(a, trfrag<TG_LD>(Ys, ks, 16 * nt, lane), acc[nt]);
    }
    float* out = partial + (size_t)chunk * E * 64;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(size_t)(e0 + 16 * wid + 4 * g + r) * 64 + 16 * nt + c16] = acc[nt][r];
    if (tid < 64) {
        if (csx) csx[(size_t)chunk * E + e0 + tid] = cs[0][0][tid] + cs[0][1][tid] + cs[0][2][tid] + cs[0][3][tid];
        if (csy && e0 == 0) csy[(size_t)chunk * 64 + tid] = cs[1][0][tid] + cs[1][1][tid] + cs[1][2][tid] + cs[1][3][tid];
    }
}

// ---------------------------------------------------------------------------------------------
// LayerNorm backward with trainable affine: dx (+ dres) as ln_bwd, plus per-block partial sums of
// d gamma = sum_r dy*xhat, d beta = sum_r dy, and the f32 column sums of dres (the gradient of the
// adapter's up-projection bias: summing its bf16 copy instead loses the cancellation-heavy sum).
// Block = 32 rows = 8 waves x 4 rows (1600 waves at T = 6400: the 64-row / 4-wave form left 156 CUs idle and
// ran 4x slower than the plain LayerNorm backward); partial[block][3][E].
constexpr int LNA_ROWS = 32;
constexpr int LNA_WAVES = 8;
constexpr int LNA_MAXV = 4;
template <typename ST>
__global__ __launch_bounds__(64 * LNA_WAVES) void ln_bwd_affine_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                            const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                            const float* __restrict__ gamma, const float* dres, float* dx,
                                                            bf16* __restrict__ dx_bf16, float* __restrict__ partial, int rows,
                                                            int E) {
    extern __shared__ float red[];     // [LNA_WAVES - 1][3][E]
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    float4 ag[LNA_MAXV], ab[LNA_MAXV], ar[LNA_MAXV];      // sums of dy*xhat, dy, dres
#pragma unroll
    for (int i = 0; i < LNA_MAXV; ++i) {
        ag[i] = make_float4(0.f, 0.f, 0.f, 0.f); ab[i] = make_float4(0.f, 0.f, 0.f, 0.f); ar[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // A wave walks its LNA_ROWS / LNA_WAVES rows with the NEXT row's operands already requested (processed one after the other
    // each row paid a full HBM round trip before its reductions could start: 27.8 us for 88 MB in step).  The walk is unrolled and
    // no load sits inside a bounds branch: rows beyond `rows` / columns beyond E read a clamped address and are masked, gamma is
    // loaded once, the next row's mean / rstd travel with its operands, and the next row is IN before this row's (conditional)
    // stores go out -- otherwise hipcc waits with vmcnt(0) at the next use, which on gfx950 also waits for those stores.
    constexpr int RPW = LNA_ROWS / LNA_WAVES;
    const float* rsrc = dres ? dres : x;
    const bool has_res = dres != nullptr;
    bool cok[LNA_MAXV];
    int cc[LNA_MAXV];
    float4 gv[LNA_MAXV];
#pragma unroll
    for (int i = 0; i < LNA_MAXV; ++i) {
        const int c = lane * 4 + i * 256;
        cok[i] = c < E; cc[i] = cok[i] ? c : 0;
        gv[i] = *reinterpret_cast<const float4*>(gamma + cc[i]);
    }
    float4 nd[LNA_MAXV], nx[LNA_MAXV], nr[LNA_MAXV];
    float nmean, nrstd;
    auto request = [&](int row) {                 // row already clamped into [0, rows)
        const size_t base = (size_t)row * E;
#pragma unroll
        for (int i = 0; i < LNA_MAXV; ++i) {
            nd[i] = *reinterpret_cast<const float4*>(dy + base + cc[i]);
            nx[i] = *reinterpret_cast<const float4*>(x + base + cc[i]);
            nr[i] = *reinterpret_cast<const float4*>(rsrc + base + cc[i]);
        }
        nmean = mean_in[row]; nrstd = rstd_in[row];
    };
    const int row_first = blockIdx.x * LNA_ROWS + wid;
    request(min(row_first, rows - 1));
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
        const int row = row_first + k * LNA_WAVES;
        const bool rok = row < rows;
        const float mean = nmean, rstd = nrstd;
        const size_t base = (size_t)row * E;
        float4 cd[LNA_MAXV], cx[LNA_MAXV], cr[LNA_MAXV];
#pragma unroll
        for (int i = 0; i < LNA_MAXV; ++i) { cd[i] = nd[i]; cx[i] = nx[i]; cr[i] = has_res ? nr[i] : make_float4(0.f, 0.f, 0.f, 0.f); }
        if (k + 1 < RPW) request(min(row + LNA_WAVES, rows - 1));
        float4 gd[LNA_MAXV], xh[LNA_MAXV];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < LNA_MAXV; ++i) {
            const bool on = rok && cok[i];
            const float4 d = cd[i];
            const float4 xv = cx[i];
            const float4 g = gv[i];
            xh[i] = make_float4((xv.x - mean) * rstd, (xv.y - mean) * rstd, (xv.z - mean) * rstd, (xv.w - mean) * rstd);
            if (on) {
                ag[i].x += d.x * xh[i].x; ag[i].y += d.y * xh[i].y; ag[i].z += d.z * xh[i].z; ag[i].w += d.w * xh[i].w;
                ab[i].x += d.x; ab[i].y += d.y; ab[i].z += d.z; ab[i].w += d.w;
                ar[i].x += cr[i].x; ar[i].y += cr[i].y; ar[i].z += cr[i].z; ar[i].w += cr[i].w;
            }
            gd[i] = make_float4(d.x * g.x, d.y * g.y, d.z * g.z, d.w * g.w);
            s1 += cok[i] ? gd[i].x + gd[i].y + gd[i].z + gd[i].w : 0.f;
            s2 += cok[i] ? gd[i].x * xh[i].x + gd[i].y * xh[i].y + gd[i].z * xh[i].z + gd[i].w * xh[i].w : 0.f;
        }
        const float m1 = wave_sum(s1) / (float)E, m2 = wave_sum(s2) / (float)E;
        __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0), visible to the compiler: the next row is in, nothing is pending behind the stores
#pragma unroll
        for (int i = 0; i < LNA_MAXV; ++i) {
            if (rok && cok[i]) {
                const int c = lane * 4 + i * 256;
                float4 o;
                o.x = rstd * (gd[i].x - m1 - xh[i].x * m2); o.y = rstd * (gd[i].y - m1 - xh[i].y * m2);
                o.z = rstd * (gd[i].z - m1 - xh[i].z * m2); o.w = rstd * (gd[i].w - m1 - xh[i].w * m2);
                o.x += cr[i].x; o.y += cr[i].y; o.z += cr[i].z; o.w += cr[i].w;
                if (dx) *reinterpret_cast<float4*>(dx + base + c) = o;       // (the engine consumes only the stored-type copy)
                if (dx_bf16) st_store4<ST>(dx_bf16, base + c, o.x, o.y, o.z, o.w);
            }
        }
    }
    // combine the waves' column sums (fixed order), write this block's partial [3][E]
    if (wid > 0) {
#pragma unroll
        for (int i = 0; i < LNA_MAXV; ++i) {
            const int c = lane * 4 + i * 256;
            if (c < E) {
                *reinterpret_cast<float4*>(red + ((size_t)(wid - 1) * 3 + 0) * E + c) = ag[i];
                *reinterpret_cast<float4*>(red + ((size_t)(wid - 1) * 3 + 1) * E + c) = ab[i];
                *reinterpret_cast<float4*>(red + ((size_t)(wid - 1) * 3 + 2) * E + c) = ar[i];
            }
        }
    }
    __syncthreads();
    if (wid == 0) {
#pragma unroll
        for (int i = 0; i < LNA_MAXV; ++i) {
            const int c = lane * 4 + i * 256;
            if (c < E) {
                float4 g = ag[i], b = ab[i], r = ar[i];
                for (int w = 0; w < LNA_WAVES - 1; ++w) {
                    const float4 g2 = *reinterpret_cast<const float4*>(red + ((size_t)w * 3 + 0) * E + c);
                    const float4 b2 = *reinterpret_cast<const float4*>(red + ((size_t)w * 3 + 1) * E + c);
                    const float4 r2 = *reinterpret_cast<const float4*>(red + ((size_t)w * 3 + 2) * E + c);
                    g.x += g2.x; g.y += g2.y; g.z += g2.z; g.w += g2.w;
                    b.x += b2.x; b.y += b2.y; b.z += b2.z; b.w += b2.w;
                    r.x += r2.x; r.y += r2.y; r.z += r2.z; r.w += r2.w;
                }
                *reinterpret_cast<float4*>(partial + ((size_t)blockIdx.x * 3 + 0) * E + c) = g;
                *reinterpret_cast<float4*>(partial + ((size_t)blockIdx.x * 3 + 1) * E + c) = b;
                *reinterpret_cast<float4*>(partial + ((size_t)blockIdx.x * 3 + 2) * E + c) = r;
            }
        }
    }
}

// out[l*out_layer + i] += sum_c partial[l*partial_layer + c*n + i].  Block = 64 columns x 4 chunk groups
// (group g sums chunks c = g, g+4, ... in order; the 4 group sums are combined in a fixed order): deterministic.
constexpr int CR_COLS = 64, CR_GROUPS = 4;
__device__ __forceinline__ float colsum_groups(const float* __restrict__ p, int chunks, size_t stride, int col, int g,
                                               float (*red)[CR_COLS]) {
    float s0 = 0.f, s1 = 0.f;
    int c = g;
    for (; c + CR_GROUPS < chunks; c += 2 * CR_GROUPS) { s0 += p[(size_t)c * stride + col]; s1 += p[(size_t)(c + CR_GROUPS) * stride + col]; }
    if (c < chunks) s0 += p[(size_t)c * stride + col];
    red[g][threadIdx.x & (CR_COLS - 1)] = s0 + s1;
    __syncthreads();
    return (red[0][threadIdx.x & (CR_COLS - 1)] + red[1][threadIdx.x & (CR_COLS - 1)]) +
           (red[2][threadIdx.x & (CR_COLS - 1)] + red[3][threadIdx.x & (CR_COLS - 1)]);
}

__global__ __launch_bounds__(256) void colsum_reduce_kernel(const float* __restrict__ partial, int chunks, int n, float* out,
                                                            size_t partial_layer, size_t out_layer) {
    __shared__ float red[CR_GROUPS][CR_COLS];
    const int i = blockIdx.x * CR_COLS + (threadIdx.x & (CR_COLS - 1)), g = threadIdx.x >> 6;
    const int col = i < n ? i : n - 1;
    const float s = colsum_groups(partial + (size_t)blockIdx.y * partial_layer, chunks, (size_t)n, col, g, red);
    if (g == 0 && i < n) out[(size_t)blockIdx.y * out_layer + i] += s;
}

// partial[l][block][3][n] -> out0/out1/out2[l*out_layer + i] += sum over blocks
__global__ __launch_bounds__(256) void colsum_reduce3_kernel(const float* __restrict__ partial, int chunks, int n, float* o0, float* o1,
                                                             float* o2, size_t partial_layer, size_t out_layer) {
    __shared__ float red[CR_GROUPS][CR_COLS];
    const int i = blockIdx.x * CR_COLS + (threadIdx.x & (CR_COLS - 1)), g = threadIdx.x >> 6;
    const int col = i < 3 * n ? i : 3 * n - 1;
    const float s = colsum_groups(partial + (size_t)blockIdx.y * partial_layer, chunks, (size_t)3 * n, col, g, red);
    if (g == 0 && i < 3 * n) {
        const int which = i / n, e = i - which * n;
        float* o = which == 0 ? o0 : (which == 1 ? o1 : o2);
        o[(size_t)blockIdx.y * out_layer + e] += s;
    }
}

// Adapter chain: g_down[j][e] += G_down[e][j] ; g_up[e][j] += G_up[e][j]   (G already chunk-reduced)
__global__ void chain_adapter_kernel(const float* __restrict__ Gd, const float* __restrict__ Gu, float* g_down, float* g_up,
                                     int E, size_t g_layer, size_t param_layer) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 64 * E) return;
    const size_t l = blockIdx.y;
    const int e = idx >> 6, j = idx & 63;
    g_down[l * param_layer + (size_t)j * E + e] += Gd[l * g_layer + idx];
    g_up[l * param_layer + idx] += Gu[l * g_layer + idx];
}

// Compacter chain: dH -> d W_left / d W_right of both PHM layers (compacter_model.py:302-308 differentiated).
//   dH_down[e][j] = Gd[e][j]  (e = a*Fi+k, j = c*16+p) ; dH_up[j][e] = Gu[e][j] (j = a*16+k, e = c*Fi+p)
//   0: d dWl[i][k] = sum_{a,c,p} Gd[a*Fi+k][c*16+p] rule[i][a][c] dWr[i][p]      3: d uWr[i][p] = sum_{a,c,k} Gu[c*Fi+p][a*16+k] rule[i][a][c] uWl[i][k]
//   1: d dWr[i][o] = sum_{a,c,k} Gd[a*Fi+k][c*16+o] rule[i][a][c] dWl[i][k]      2: d uWl[i][o] = sum_{a,c,p} Gu[c*Fi+p][a*16+o] rule[i][a][c] uWr[i][p]
// One 16-wave block per (tensor, layer), all four PHM slices i at once.  A wave reads whole 64-float rows of G (lane = column:
// 256 coalesced bytes per request, every row fetched once per block) -- tensors 0 / 3 contract a row against a per-lane
// coefficient and reduce it over the wave; tensors 1 / 2 accumulate per lane over the rows and meet through LDS.  Every output is
// a fixed-order sum: deterministic.  (Round 4; the one-thread-per-output form walked 256 strided loads in sequence: 43 us.)
constexpr int CC_WAVES = 16;
__global__ __launch_bounds__(64 * CC_WAVES) void chain_compacter_kernel(const float* __restrict__ Gd, const float* __restrict__ Gu,
                                                              const float* __restrict__ rule, const float* __restrict__ params,
                                                              float* grads, int E, size_t g_layer, size_t param_layer,
                                                              size_t off_dWl, size_t off_dWr, size_t off_uWl, size_t off_uWr) {
    __shared__ float part[CC_WAVES][4][16];
    const size_t l = blockIdx.y;
    const int which = blockIdx.x;
    const int Fi = E / 4;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hi = lane >> 4, lo = lane & 15;
    const float* P = params + l * param_layer; float* Gp = grads + l * param_layer;
    const bool down = which < 2;
    const float* G = (down ? Gd : Gu) + l * g_layer;
    if (which == 0 || which == 3) {
        // long output index q (k resp. p), short contracted index lo (p resp. k), rule index pair (x, hi): rows x*Fi + q, x = 0..3
        const float* vshort = P + (which == 0 ? off_dWr : off_uWl);            // [i][16]
        float m[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const float r = (which == 0) ? rule[i * 16 + x * 4 + hi] : rule[i * 16 + hi * 4 + x];      // rule[i][a][c]
                m[i][x] = r * vshort[i * 16 + lo];
            }
        float* out = Gp + (which == 0 ? off_dWl : off_uWr);
        for (int q0 = w; q0 < Fi; q0 += 2 * CC_WAVES) {
            float xr[2][4];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int q = min(q0 + u * CC_WAVES, Fi - 1);
#pragma unroll
                for (int x = 0; x < 4; ++x) xr[u][x] = G[(size_t)(x * Fi + q) * 64 + lane];
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int q = q0 + u * CC_WAVES;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float v = xr[u][0] * m[i][0] + xr[u][1] * m[i][1] + xr[u][2] * m[i][2] + xr[u][3] * m[i][3];
                    v = wave_sum(v);
                    if (lane == 0 && q < Fi) out[(size_t)i * Fi + q] += v;
                }
            }
        }
    } else {
        // 16 outputs lo per slice; lane column = (hi, lo); rows x*Fi + q contracted with rule[i][.][.] (pair (x, hi)) and vlong[i][q]
        const float* vlong = P + (which == 1 ? off_dWl : off_uWr);             // [i][Fi]
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int x = 0; x < 4; ++x) {
            float r[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] = (which == 1) ? rule[i * 16 + x * 4 + hi] : rule[i * 16 + hi * 4 + x];
            for (int q0 = w; q0 < Fi; q0 += 4 * CC_WAVES) {
                float xr[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) xr[u] = G[(size_t)(x * Fi + min(q0 + u * CC_WAVES, Fi - 1)) * 64 + lane];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int q = q0 + u * CC_WAVES;
                    if (q < Fi) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[i] += xr[u] * r[i] * vlong[(size_t)i * Fi + q];
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v = acc[i];
            v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
            if (lane < 16) part[w][i][lane] = v;
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            const int i = threadIdx.x >> 4, o = threadIdx.x & 15;
            float t = 0.f;
            for (int ww = 0; ww < CC_WAVES; ++ww) t += part[ww][i][o];
            Gp[(which == 1 ? off_dWr : off_uWl) + (size_t)i * 16 + o] += t;
        }
    }
}

}  // namespace

int pevit_tn_chunks(int T) { return ceil_div(T, TG_ROWS); }
int pevit_lna_blocks(int rows) { return ceil_div(rows, LNA_ROWS); }

int pevit_launch_prep_adapter(const float* w_down, const float* w_up, BottleneckPanels pan, int E, int layers, LayerStrides st,
                              hipStream_t s, int f32) {
    if (f32) hipLaunchKernelGGL(prep_adapter_kernel<float>, dim3(ceil_div(64 * E, 256), layers), dim3(256), 0, s, w_down, w_up, pan, E, st);
    else hipLaunchKernelGGL(prep_adapter_kernel<bf16>, dim3(ceil_div(64 * E, 256), layers), dim3(256), 0, s, w_down, w_up, pan, E, st);
    LAUNCH_OK("prep_adapter_kernel");
    return 0;
}
int pevit_launch_prep_compacter(const PrepCompacterArgs& a, hipStream_t s) {
    const int E = a.E;
    if (E % 4) { pevit_set_error("prep_compacter: width %d not divisible by 4", E); return -1; }
    if (a.f32) hipLaunchKernelGGL(prep_compacter_kernel<float>, dim3(ceil_div(64 * E, 256), a.layers), dim3(256), 0, s, a.rule, a.dWl, a.dWr, a.uWl,
                                  a.uWr, a.pan, E, a.st);
    else hipLaunchKernelGGL(prep_compacter_kernel<bf16>, dim3(ceil_div(64 * E, 256), a.layers), dim3(256), 0, s, a.rule, a.dWl, a.dWr, a.uWl,
                            a.uWr, a.pan, E, a.st);
    LAUNCH_OK("prep_compacter_kernel");
    return 0;
}
int pevit_launch_tn_gemm64(const TnGemm64Args& a, hipStream_t s) {
    if (a.E % 64 || (a.ldx % 8) || (a.ldy % 8)) { pevit_set_error("tn_gemm64: bad shape E=%d ldx=%d ldy=%d", a.E, a.ldx, a.ldy); return -1; }
    hipLaunchKernelGGL(tn_gemm64_kernel, dim3(ceil_div(a.T, TG_ROWS) * (a.E / 64)), dim3(256), 0, s, a.X, a.ldx, a.Y, a.ldy, a.partial, a.csx,
                       a.csy, a.T, a.E);
    LAUNCH_OK("tn_gemm64_kernel");
    return 0;
}
template <typename ST>
static int launch_ln_bwd_affine(const LnBwdAffineArgs& a, hipStream_t s) {
    const int rows = a.rows, E = a.E;
    if (E % 4 || E > 256 * LNA_MAXV) { pevit_set_error("ln_bwd_affine: unsupported width %d", E); return -1; }
    const size_t lds = (size_t)(LNA_WAVES - 1) * 3 * E * sizeof(float);      // 64.5 KiB at E = 768
    constexpr int maxlds = (LNA_WAVES - 1) * 3 * 256 * LNA_MAXV * (int)sizeof(float);
    if (reserve_lds<ln_bwd_affine_kernel<ST>, maxlds>("ln_bwd_affine")) return -1;
    hipLaunchKernelGGL(ln_bwd_affine_kernel<ST>, dim3(ceil_div(rows, LNA_ROWS)), dim3(64 * LNA_WAVES), lds, s, a.dy, a.x, a.mean, a.rstd, a.gamma,
                       a.dres, a.dx, a.dx_bf16, a.partial, rows, E);
    LAUNCH_OK("ln_bwd_affine_kernel");
    return 0;
}
int pevit_launch_ln_bwd_affine(const LnBwdAffineArgs& a, hipStream_t s) {
    return a.f32 == 0 ? launch_ln_bwd_affine<bf16>(a, s) : launch_ln_bwd_affine<float>(a, s);      // (named in the order the code object lists them)
}
int pevit_launch_colsum_reduce(const float* partial, int chunks, int n, float* out, int layers, size_t partial_layer,
                               size_t out_layer, hipStream_t s) {
    hipLaunchKernelGGL(colsum_reduce_kernel, dim3(ceil_div(n, CR_COLS), layers), dim3(256), 0, s, partial, chunks, n, out,
                       partial_layer, out_layer);
    LAUNCH_OK("colsum_reduce_kernel");
    return 0;
}
int pevit_launch_colsum_reduce3(const ColsumReduce3Args& a, hipStream_t s) {
    hipLaunchKernelGGL(colsum_reduce3_kernel, dim3(ceil_div(3 * a.n, CR_COLS), a.layers), dim3(256), 0, s, a.partial, a.chunks, a.n, a.o0, a.o1, a.o2,
                       a.partial_layer, a.out_layer);
    LAUNCH_OK("colsum_reduce3_kernel");
    return 0;
}
int pevit_launch_chain_adapter(const float* Gd, const float* Gu, float* g_down, float* g_up, int E, int layers, size_t g_layer,
                               size_t param_layer, hipStream_t s) {
    hipLaunchKernelGGL(chain_adapter_kernel, dim3(ceil_div(64 * E, 256), layers), dim3(256), 0, s, Gd, Gu, g_down, g_up, E,
                       g_layer, param_layer);
    LAUNCH_OK("chain_adapter_kernel");
    return 0;
}
int pevit_launch_chain_compacter(const ChainCompacterArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(chain_compacter_kernel, dim3(4, a.layers), dim3(64 * CC_WAVES), 0, s, a.Gd, a.Gu, a.rule, a.params, a.grads, a.E, a.g_layer,
                       a.param_layer, a.off_dWl, a.off_dWr, a.off_uWl, a.off_uWr);
    LAUNCH_OK("chain_compacter_kernel");
    return 0;
}
