// Single-kernel entry points (parity tests, profiling): each fills a launcher's parameters from its arguments and launches.  They are
// context-free, and this unit sees kernels.h only, not the engine's context (host_ctx.h).
#include <string.h>

#include "../../include/pevit_hip.h"
#include "common.h"
#include "kernels.h"
#include "gemm_plan.h"

// What two context calls reach into when they are given no context (host_ctx.h declares both): pevit_tune(nullptr, ...) sets this
// tune, pevit_streamk_error(nullptr, ...) reads the error word of this workspace.
namespace pevit_host __attribute__((visibility("hidden"))) {

GemmTune g_default_tune;

// stream-K workspace of the context-free entry point (tests / microbenchmarks): allocated on first use
int op_sk_workspace(GemmParams& p) {
    static char* ws = nullptr;
    const int slots = pevit_gemm_sk_slots();
    const size_t flag_bytes = align_up((size_t)(PEVIT_SK_MAX_SLOTS + 1) * 4, 256);
    if (!ws) {
        HIP_OK(hipMalloc((void**)&ws, flag_bytes + (size_t)slots * PEVIT_SK_SLAB_FLOATS * 4));
        HIP_OK(hipMemset(ws, 0, flag_bytes));
    }
    p.sk_flag = reinterpret_cast<unsigned*>(ws); p.sk_slab = reinterpret_cast<float*>(ws + flag_bytes); p.sk_slots = slots;
    return 0;
}

}  // namespace pevit_host

using namespace pevit_host;

static GemmParams gp(const void* A, int lda, const void* B, int ldb, int Nb, int M, int N, int K) {
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.A = (const bf16*)A; p.lda = lda; p.B = B; p.ldb = ldb; p.Nb = Nb; p.M = M; p.N = N; p.K = K;
    return p;
}

extern "C" int pevit_op_gemm(void* stream, int epi, const void* A, int lda, const void* Bm, int ldb, int b_rows, int M,
                             int N, int K, const float* bias, const float* resid, int ldr, float* outf, int ldo,
                             void* outb, int ldob, void* outb2, int ldob2, const void* aux, int ldaux,
                             size_t head_stride, int E, int H, int tokens) {
    GemmParams p = gp(A, lda, Bm, ldb, b_rows, M, N, K);
    p.bias = bias; p.resid = resid; p.ldr = ldr; p.outf = outf; p.ldo = ldo; p.outb = (bf16*)outb; p.ldob = ldob;
    p.outb2 = (bf16*)outb2; p.ldob2 = ldob2; p.aux = (const bf16*)aux; p.ldaux = ldaux; p.head_stride = head_stride;
    p.E = E; p.H = H; p.Ntok = tokens;
    if (g_default_tune.streamk && op_sk_workspace(p)) return -1;
    return pevit_launch_gemm(epi, p, g_default_tune, (hipStream_t)stream);
}
extern "C" int pevit_op_gemm_fp8(void* stream, int epi, const void* A, int lda, const void* Bcodes, int ldb, int b_rows,
                                 const float* bscale, const float* oscale, int M, int N, int K, const float* bias,
                                 const float* resid, int ldr, float* outf, int ldo, void* outb, int ldob, void* outb2,
                                 int ldob2, const void* aux, int ldaux, size_t head_stride, int E, int H, int tokens) {
    GemmParams p = gp(A, lda, Bcodes, ldb, b_rows, M, N, K);
    p.b_fp8 = 1; p.bscale = bscale; p.oscale = oscale;
    p.bias = bias; p.resid = resid; p.ldr = ldr; p.outf = outf; p.ldo = ldo; p.outb = (bf16*)outb; p.ldob = ldob;
    p.outb2 = (bf16*)outb2; p.ldob2 = ldob2; p.aux = (const bf16*)aux; p.ldaux = ldaux; p.head_stride = head_stride;
    p.E = E; p.H = H; p.Ntok = tokens;
    return pevit_launch_gemm(epi, p, g_default_tune, (hipStream_t)stream);
}
// fp8 x fp8 form (PEVIT_W_FP8_ACT): A = unscaled e4m3 codes as written by pevit_op_cast_fp8
extern "C" int pevit_op_gemm_f8a(void* stream, int epi, const void* Acodes, int lda, const void* Bcodes, int ldb, int b_rows,
                                 const float* bscale, int M, int N, int K, const float* bias, const float* resid, int ldr,
                                 float* outf, int ldo, void* outb, int ldob, void* outb2, int ldob2, int out2_fp8,
                                 size_t head_stride, int E, int H, int tokens) {
    GemmParams p = gp(Acodes, lda, Bcodes, ldb, b_rows, M, N, K);
    p.b_fp8 = 1; p.a_fp8 = 1; p.bscale = bscale; p.out2_fp8 = out2_fp8;
    p.bias = bias; p.resid = resid; p.ldr = ldr; p.outf = outf; p.ldo = ldo; p.outb = (bf16*)outb; p.ldob = ldob;
    p.outb2 = (bf16*)outb2; p.ldob2 = ldob2; p.head_stride = head_stride; p.E = E; p.H = H; p.Ntok = tokens;
    return pevit_launch_gemm(epi, p, g_default_tune, (hipStream_t)stream);
}
extern "C" int pevit_op_cast_fp8(void* stream, const float* src, void* codes, int rows, int cols) {
    return pevit_launch_cast_fp8(src, (unsigned char*)codes, (size_t)rows, cols, (hipStream_t)stream);
}
extern "C" int pevit_op_quant_fp8(void* stream, const float* W, int rows, int cols, void* codes, float* scales,
                                  void* codes_t) {
    if (pevit_launch_quant_rows_fp8(W, rows, cols, (unsigned char*)codes, cols, scales, 0, 1.0f, (hipStream_t)stream)) return -1;
    if (!codes_t) return 0;
    return pevit_launch_quant_transpose_fp8(W, rows, cols, scales, (unsigned char*)codes_t, rows, 0, 1.0f, (hipStream_t)stream);
}
extern "C" int pevit_op_dequant_fp8(void* stream, const void* codes, const float* scales, int rows, int cols, float* out) {
    return pevit_launch_dequant_rows_fp8((const unsigned char*)codes, cols, scales, rows, cols, out, (hipStream_t)stream);
}
extern "C" int pevit_op_ln_fwd(void* stream, const float* x, const float* gamma, const float* beta, int rows, int E,
                               void* y_bf16, float* y_f32, float* mean, float* rstd) {
    LnFwdArgs a;
    a.x = x; a.gamma = gamma; a.beta = beta; a.rows = rows; a.E = E; a.y_bf16 = (bf16*)y_bf16; a.y_f32 = y_f32; a.mean = mean; a.rstd = rstd;
    return pevit_launch_ln_fwd(a, (hipStream_t)stream);
}
extern "C" int pevit_op_ln_bwd_scaled(void* stream, const float* dy, const float* x, const float* mean, const float* rstd,
                                      const float* gamma, const float* dres, float* dx, void* dx_bf16, int rows, int E,
                                      const float* bf16_colscale) {
    LnBwdArgs a;
    a.dy = dy; a.x = x; a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.dres = dres; a.dx_out = dx; a.dx_bf16 = (bf16*)dx_bf16;
    a.rows = rows; a.E = E; a.bf16_colscale = bf16_colscale;
    return pevit_launch_ln_bwd(a, (hipStream_t)stream);
}
extern "C" int pevit_op_ln_bwd(void* stream, const float* dy, const float* x, const float* mean, const float* rstd,
                               const float* gamma, const float* dres, float* dx, void* dx_bf16, int rows, int E) {
    return pevit_op_ln_bwd_scaled(stream, dy, x, mean, rstd, gamma, dres, dx, dx_bf16, rows, E, nullptr);
}
extern "C" int pevit_op_attn_fwd(void* stream, const void* q, const void* k, const void* v, void* out, int ldo,
                                 float* lse, int B, int H, int N) {
    AttnArgs a;
    a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v; a.out = (bf16*)out; a.ldo = ldo; a.lse = lse; a.B = B; a.H = H; a.N = N;
    return pevit_launch_attn_fwd(a, (hipStream_t)stream);
}
extern "C" int pevit_op_attn_fwd_causal(void* stream, const void* q, const void* k, const void* v, void* out, int ldo, int B, int H, int N) {
    AttnArgs a;
    a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v; a.out = (bf16*)out; a.ldo = ldo; a.B = B; a.H = H; a.N = N;
    return pevit_launch_attn_fwd_causal(a, (hipStream_t)stream);
}
extern "C" int pevit_op_attn_bwd(void* stream, const void* q, const void* k, const void* v, const void* out, int ldo,
                                 const void* dout, int lddo, const float* lse, void* dqkv, int ld, int B, int H, int N) {
    AttnArgs a;      // (out and lse are only read by the backward)
    a.q = (const bf16*)q; a.k = (const bf16*)k; a.v = (const bf16*)v; a.out = (bf16*)const_cast<void*>(out); a.ldo = ldo;
    a.lse = const_cast<float*>(lse); a.B = B; a.H = H; a.N = N; a.dout = (const bf16*)dout; a.lddo = lddo; a.dqkv = (bf16*)dqkv; a.ld = ld;
    return pevit_launch_attn_bwd(a, (hipStream_t)stream);
}
extern "C" int pevit_op_cast_bf16(void* stream, const float* src, void* dst, size_t n, float scale) {
    return pevit_launch_cast_bf16(src, (bf16*)dst, n, scale, (hipStream_t)stream);
}
extern "C" int pevit_op_delta_add(void* stream, void* qbuf, void* vbuf, const float* t, const void* q16,
                                  const float* bias, float ascale, int B, int N, int E) {
    DeltaAddArgs a;
    a.qbuf = (bf16*)qbuf; a.vbuf = (bf16*)vbuf; a.t = t; a.q16 = (const bf16*)q16; a.bias = bias; a.ascale = ascale; a.B = B; a.N = N; a.E = E;
    return pevit_launch_delta_add(a, (hipStream_t)stream);
}
extern "C" int pevit_op_attn_fwd_delta(void* stream, void* q, const void* k, void* v, const float* t, const void* q16, const float* bias,
                                       float ascale, void* out, int ldo, float* lse, int B, int H, int N) {
    AttnFwdDeltaArgs a;
    a.q = (bf16*)q; a.k = (const bf16*)k; a.v = (bf16*)v; a.t = t; a.q16 = (const bf16*)q16; a.bias = bias; a.ascale = ascale;
    a.out = (bf16*)out; a.ldo = ldo; a.lse = lse; a.B = B; a.H = H; a.N = N;
    a.nosave = lse == nullptr;      // no lse buffer: the inference form (q, v are left as they are)
    return pevit_launch_attn_fwd_delta(a, (hipStream_t)stream);
}
static int seg_args(AttnSiteSegArgs& a, const char* who, int nseg, const pevit_op_segment* segs) {
    if (!segs || nseg < 1 || nseg > PEVIT_MAX_SEGMENTS) { pevit_set_error("%s: %d segments outside [1,%d]", who, nseg, PEVIT_MAX_SEGMENTS); return -1; }
    a.nseg = nseg;
    for (int i = 0; i < nseg; ++i) {
        a.seg[i].first = segs[i].first; a.seg[i].count = segs[i].count; a.seg[i].tcol = segs[i].tcol;
        a.seg[i].q16 = (const bf16*)segs[i].q16_bf16; a.seg[i].bias = segs[i].bias;
    }
    return 0;
}
extern "C" int pevit_op_delta_add_seg(void* stream, void* qbuf, void* vbuf, const float* t, int tpitch, float ascale, int B, int H, int N,
                                      int nseg, const pevit_op_segment* segs) {
    AttnSiteSegArgs a;
    a.q = (bf16*)qbuf; a.v = (bf16*)vbuf; a.t = t; a.tpitch = tpitch; a.ascale = ascale; a.B = B; a.H = H; a.N = N;
    if (seg_args(a, "delta_add_seg", nseg, segs)) return -1;
    return pevit_launch_delta_add_seg(a, (hipStream_t)stream);
}
extern "C" int pevit_op_attn_fwd_delta_seg(void* stream, const void* q, const void* k, const void* v, const float* t, int tpitch,
                                           float ascale, void* out, int ldo, int B, int H, int N, int nseg, const pevit_op_segment* segs) {
    AttnSiteSegArgs a;      // (q and v are only read by the fused inference form)
    a.q = (bf16*)const_cast<void*>(q); a.k = (const bf16*)k; a.v = (bf16*)const_cast<void*>(v); a.t = t; a.tpitch = tpitch; a.ascale = ascale;
    a.out = (bf16*)out; a.ldo = ldo; a.B = B; a.H = H; a.N = N;
    if (seg_args(a, "attn_fwd_delta_seg", nseg, segs)) return -1;
    return pevit_launch_attn_fwd_delta_seg(a, (hipStream_t)stream);
}
// the segmented inference launch of the fused post-MLP adapter forward (adapter_fused.hip): AdapterFwdSegArgs by name
extern "C" int pevit_op_adapter_fwd_seg(void* stream, const pevit_adapter_fwd_seg_args* a) {
    const char* who = "adapter_fwd_seg";
    if (!a) { pevit_set_error("%s: null argument struct", who); return -1; }
    if (!a->segs || a->nseg < 1 || a->nseg > PEVIT_MAX_SEGMENTS) { pevit_set_error("%s: %d segments outside [1,%d]", who, a->nseg, PEVIT_MAX_SEGMENTS); return -1; }
    AdapterFwdSegArgs p;
    p.act_kind = a->act_kind; p.E = a->E; p.hraw = a->hraw; p.bpr = a->bpr; p.x_mid = a->x_mid; p.x_out = a->x_out; p.nseg = a->nseg;
    for (int i = 0; i < a->nseg; ++i) {
        const pevit_adapter_seg& g = a->segs[i];
        AdapterSegment& o = p.seg[i];
        o.first = g.first; o.end = g.end; o.gamma = g.gamma; o.beta = g.beta; o.wd = (const bf16*)g.wd; o.b_down = g.b_down;
        o.wu = (const bf16*)g.wu; o.b_up = g.b_up;
    }
    return pevit_launch_adapter_fwd_seg(p, (hipStream_t)stream);
}
extern "C" int pevit_debug_occupy(void* stream, int workgroups, int lds_bytes, double microseconds) {
    return pevit_launch_occupy(workgroups, lds_bytes, microseconds, (hipStream_t)stream);
}
extern "C" int pevit_debug_timeline(void* buf) { pevit_attn_delta_set_timeline(buf); return 0; }
extern "C" int pevit_op_attn_delta_hpw(int B, int H, int N) { return pevit_attn_delta_hpw(B, H, N); }
extern "C" int pevit_op_attn_probs(void* stream, const void* q, const void* k, const float* lse, float* out, int B, int H, int N,
                                   int average) {
    AttnArgs a;      // (lse is only read)
    a.q = (const bf16*)q; a.k = (const bf16*)k; a.lse = const_cast<float*>(lse); a.probs = out; a.B = B; a.H = H; a.N = N; a.average = average;
    return pevit_launch_attn_probs(a, (hipStream_t)stream);
}
extern "C" int pevit_op_lowrank_u(void* stream, const void* dqkv, int ld, const void* qT, float* u32, void* u_cols, int B,
                                  int H, int N, int E) {
    LowrankArgs a;
    a.dqkv = (const bf16*)dqkv; a.ld = ld; a.qT = (const bf16*)qT; a.u32 = u32; a.u_bf16_cols = (bf16*)u_cols; a.B = B; a.H = H; a.N = N; a.E = E;
    return pevit_launch_lowrank_u(a, (hipStream_t)stream);
}
extern "C" int pevit_op_lowrank_grad(void* stream, const void* xn, int ldx, const float* u32, const void* dqkv, int ld,
                                     const float* t, float* partial, float* dbias_partial, int B, int H, int N, int E) {
    LowrankArgs a;      // (u32 is only read by this kernel)
    a.xn = (const bf16*)xn; a.ldx = ldx; a.u32 = const_cast<float*>(u32); a.dqkv = (const bf16*)dqkv; a.ld = ld; a.t = t; a.partial = partial;
    a.dbias_partial = dbias_partial; a.chunks = pevit_lowrank_chunks(B * N); a.B = B; a.H = H; a.N = N; a.E = E;
    return pevit_launch_lowrank_grad(a, (hipStream_t)stream);
}
extern "C" int pevit_op_lowrank_chunks(int T) { return pevit_lowrank_chunks(T); }
// ---- post-MLP adapter kernels (adapter.hip), one layer at a time
extern "C" int pevit_op_tn_chunks(int T) { return pevit_tn_chunks(T); }
extern "C" int pevit_op_lna_blocks(int rows) { return pevit_lna_blocks(rows); }
extern "C" int pevit_op_tn_gemm64(void* stream, const void* X, int ldx, const void* Y, int ldy, float* partial, float* csx,
                                  float* csy, int T, int E) {
    TnGemm64Args a;
    a.X = (const bf16*)X; a.ldx = ldx; a.Y = (const bf16*)Y; a.ldy = ldy; a.partial = partial; a.csx = csx; a.csy = csy; a.T = T; a.E = E;
    return pevit_launch_tn_gemm64(a, (hipStream_t)stream);
}
extern "C" int pevit_op_ln_bwd_affine(void* stream, const float* dy, const float* x, const float* mean, const float* rstd,
                                      const float* gamma, const float* dres, float* dx, void* dx_bf16, float* partial,
                                      int rows, int E) {
    LnBwdAffineArgs a;
    a.dy = dy; a.x = x; a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.dres = dres; a.dx = dx; a.dx_bf16 = (bf16*)dx_bf16; a.partial = partial;
    a.rows = rows; a.E = E;
    return pevit_launch_ln_bwd_affine(a, (hipStream_t)stream);
}
extern "C" int pevit_op_colsum_reduce(void* stream, const float* partial, int chunks, int n, float* out0, float* out1,
                                      float* out2) {
    if (out1 || out2) {
        if (!out1 || !out2) { pevit_set_error("colsum_reduce: give one output or three"); return -1; }
        ColsumReduce3Args a;
        a.partial = partial; a.chunks = chunks; a.n = n; a.o0 = out0; a.o1 = out1; a.o2 = out2; a.layers = 1;
        return pevit_launch_colsum_reduce3(a, (hipStream_t)stream);
    }
    return pevit_launch_colsum_reduce(partial, chunks, n, out0, 1, 0, 0, (hipStream_t)stream);
}
extern "C" int pevit_op_prep_bottleneck(void* stream, int method, const float* rule, const float* p0, const float* p1,
                                        const float* p2, const float* p3, void* wd, void* wdT, void* wu, void* wuT, int E) {
    BottleneckPanels pan{(bf16*)wd, (bf16*)wdT, (bf16*)wu, (bf16*)wuT};
    LayerStrides st{0, 0};
    if (method == PEVIT_ADAPTER) return pevit_launch_prep_adapter(p0, p1, pan, E, 1, st, (hipStream_t)stream);
    if (method == PEVIT_COMPACTER) {
        PrepCompacterArgs a;
        a.rule = rule; a.dWl = p0; a.dWr = p1; a.uWl = p2; a.uWr = p3; a.pan = pan; a.E = E; a.layers = 1; a.st = st;
        return pevit_launch_prep_compacter(a, (hipStream_t)stream);
    }
    pevit_set_error("prep_bottleneck: method %d is not a post-MLP adapter", method);
    return -1;
}
extern "C" int pevit_op_chain_bottleneck(void* stream, int method, const float* Gd, const float* Gu, const float* rule,
                                         const float* params, float* grads, int E, size_t off0, size_t off1, size_t off2,
                                         size_t off3) {
    if (method == PEVIT_ADAPTER)
        return pevit_launch_chain_adapter(Gd, Gu, grads + off0, grads + off1, E, 1, 0, 0, (hipStream_t)stream);
    if (method == PEVIT_COMPACTER) {
        ChainCompacterArgs a;
        a.Gd = Gd; a.Gu = Gu; a.rule = rule; a.params = params; a.grads = grads; a.E = E; a.layers = 1;
        a.off_dWl = off0; a.off_dWr = off1; a.off_uWl = off2; a.off_uWr = off3;
        return pevit_launch_chain_compacter(a, (hipStream_t)stream);
    }
    pevit_set_error("chain_bottleneck: method %d is not a post-MLP adapter", method);
    return -1;
}
extern "C" int pevit_op_im2col_u8(void* stream, const uint8_t* images, const float* mean3, const float* std3, void* patches_bf16, int B,
                                  int R, int P, int Kpad) {
    Im2colU8Args a;
    a.img = images; a.mean3 = mean3; a.std3 = std3; a.out = (bf16*)patches_bf16; a.B = B; a.R = R; a.P = P; a.Kp = Kpad;
    return pevit_launch_im2col_u8(a, (hipStream_t)stream);
}
extern "C" int pevit_op_im2col(void* stream, const float* images, void* patches_bf16, int B, int R, int P, int Kpad) {
    return pevit_launch_im2col(images, (bf16*)patches_bf16, B, R, P, Kpad, (hipStream_t)stream);
}
// the zero-shot head alone (zeroshot.hip): the seam its parity tests use
extern "C" int pevit_op_zeroshot_head(void* stream, const float* feat, const float* text_cd, float scale, float* probs_or_null,
                                      float* logits_or_null, int B, int D, int C) {
    ZeroshotArgs a;
    a.feat = feat; a.text = text_cd; a.scale = scale; a.probs = probs_or_null; a.logits = logits_or_null; a.B = B; a.D = D; a.C = C;
    return pevit_launch_zeroshot_head(a, (hipStream_t)stream);
}

// Every member of GemmParams by name, a tune of its own (default-constructed, the set knobs overwritten: the process-wide default tune
// is not touched) and the caller's stream-K workspace (tests/test_gpu_gemm_forms.py, tests/test_gemm_forms_host.py).
static void gemm_ex_problem(const pevit_gemm_ex_args* a, GemmParams& p, GemmTune& t) {
    p = GemmParams{};      // every member zero / null
    p.A = (const bf16*)a->A; p.lda = a->lda; p.B = a->B; p.ldb = a->ldb; p.Nb = a->b_rows;
    p.B2 = (const bf16*)a->B2; p.ldb2 = a->ldb2; p.Nb2 = a->b2_rows; p.n_fp8 = a->n_fp8;
    p.b_fp8 = a->b_fp8; p.a_fp8 = a->a_fp8; p.bscale = a->bscale; p.oscale = a->oscale;
    p.M = a->M; p.N = a->N; p.K = a->K;
    p.bias = a->bias; p.resid = a->resid; p.ldr = a->ldr;
    p.outf = a->out_f32; p.ldo = a->ldo; p.outf2 = a->out_f32_2; p.ldo2 = a->ldo2;
    p.outb = (bf16*)a->out_bf16; p.ldob = a->ldob; p.outb2 = (bf16*)a->out2_bf16; p.ldob2 = a->ldob2;
    p.aux = (const bf16*)a->aux_bf16; p.ldaux = a->ldaux;
    p.head_stride = a->head_stride; p.E = a->E; p.H = a->H; p.Ntok = a->tokens;
    p.sk_slab = a->sk_slab; p.sk_flag = a->sk_flag; p.sk_slots = a->sk_slots;
    t = GemmTune{};
    int* const knob[PEVIT_KNOB_COUNT] = {&t.config, &t.stagger, &t.big, &t.ksplit, &t.ksplit_small, &t.ksplit_stagger, &t.ksplit_mink,
                                         &t.kphase_nl, &t.kz2, &t.skinny, &t.skinny_slices, &t.streamk, &t.persistent};
    for (int i = 0; i < PEVIT_KNOB_COUNT; ++i)
        if (a->tune_set >> i & 1u) *knob[i] = a->tune[i];
}
extern "C" int pevit_op_gemm_ex(void* stream, const pevit_gemm_ex_args* a) {
    if (!a) { pevit_set_error("gemm_ex: null argument struct"); return -1; }
    GemmParams p; GemmTune t;
    gemm_ex_problem(a, p, t);
    return pevit_launch_gemm(a->epilogue, p, t, (hipStream_t)stream);
}
extern "C" int pevit_op_gemm_sk_slots(void) { return pevit_gemm_sk_slots(); }

extern "C" int pevit_debug_last_gemm_path(void) { return pevit_gemm_last_path(); }
// The plan of the problem pevit_op_gemm_ex would launch, on a device of `cus` compute units.  No HIP call, no pointer touched: the
// planner reads pointers as set / unset and as the B2 - B distance, so this runs without a GPU (tests/test_gemm_forms_host.py).
extern "C" int pevit_debug_gemm_plan(const pevit_gemm_ex_args* a, int cus, pevit_gemm_plan_info* out) {
    if (!a || !out) { pevit_set_error("gemm_plan: null argument"); return -1; }
    GemmParams p; GemmTune t;
    gemm_ex_problem(a, p, t);
    const pevit_gemm::GemmPlan pl = pevit_gemm::plan_gemm(a->epilogue, p, t, cus);
    *out = pevit_gemm_plan_info{pl.path, pl.ops, pl.cfg, pl.wm, pl.nl, pl.stag, pl.tiles, pl.grid, pl.band, pl.sk.share, pl.sk.band,
                                pl.tiles_n, pl.nslices, pl.ksl, {}};
    memcpy(out->err, pl.err, sizeof(out->err));
    if (pl.err[0]) { pevit_set_error("%s", pl.err); return -1; }
    return 0;
}
extern "C" int pevit_debug_gemm_epi_traits(int epilogue) {
    if (epilogue < EPI_QKV_HEADS || epilogue > EPI_LAST) return -1;
    const pevit_gemm::EpiTraits tr = pevit_gemm::epi_traits(epilogue);
    return (int)tr.fp8b | (int)tr.fp8a << 1 | (int)tr.skinny << 2 | (int)tr.ksplit << 3;
}
