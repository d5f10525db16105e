// The per-layer launch sequence: forward and backward walks over the residual blocks, and the attention half of a block that the
// attention seam shares with them.
#include "host_ctx.h"

namespace pevit_host {

// slot: a slot of a multi-slot context; -1: the panels of the single-adapter calls (on such a context: the rows behind the last slot
// and b.q16).  The f32 and the transposed panels are write-only on an inference-only context: every slot stores them to the same place.
static AdapterPanels panels(pevit_ctx* c, int l, int slot = -1) {
    const BlockArena& b = c->blk[l];
    AdapterPanels p;
    const size_t prow = 3 * (size_t)c->E + 64 * (size_t)(slot < 0 ? c->slots : slot);
    p.w_aug_rows = c->fp8 ? at<bf16>(c->arena, b.wpan) : eadv(c, at<bf16>(c->arena, b.wqkv), prow * c->E);
    p.ldw = c->E;
    // (an inference-only context has no wqkvT: the 64 columns go to its write-only panel, nobody reads them)
    p.wT_aug_cols = c->infer_only ? at<bf16>(c->arena, b.tsink) : eadv(c, at<bf16>(c->arena, b.wqkvT), 3 * (size_t)c->E);
    p.ldwT = c->infer_only ? 64 : c->NQ;
    p.q32 = at<float>(c->arena, b.q32);
    p.qT = at<bf16>(c->arena, b.qT);
    p.q16 = slot < 0 ? at<bf16>(c->arena, b.q16) : at<bf16>(c->arena, b.q16s + (size_t)slot * q16_slot_bytes(c));
    return p;
}

// rebuild the bf16 adapter panels of every layer from the f32 master parameters (one launch).  slot >= 0 (pevit_load_adapter_slot):
// the panels of that slot of a multi-slot context from `params`; otherwise those of the single-adapter calls from c->params
// phm_rule (Compacter, slot >= 0): the slot's frozen rule, read from the caller's buffer; the single-adapter calls read the arena's
int prep_adapters(pevit_ctx* c, hipStream_t s, int slot, const float* params, const float* phm_rule) {
    const size_t E = c->E;
    LayerStrides st;
    st.arena_bytes = c->L > 1 ? c->blk[1].wqkv - c->blk[0].wqkv : 0;
    st.param_floats = c->p_layer_stride;
    if (slot < 0) params = c->params;
    const float* lp = params + c->p_layer0;
    if (c->d.method == PEVIT_KADAPTATION) {
        const float* r = params;
        PrepKadaptArgs a;
        a.rule1_l = r; a.rule1_r = r + 1024; a.rule2_l = r + 2048; a.rule2_r = r + 3072; a.q_left = lp; a.q_right = lp + E;
        a.pan = panels(c, 0, slot); a.E = c->E; a.ascale = c->ascale; a.layers = c->L; a.st = st; a.f32 = c->f32;
        CHECK(pevit_launch_prep_kadapt(a, s));
    } else if (c->d.method == PEVIT_LORA) {
        const size_t rE = (size_t)c->d.lora_rank * E;
        PrepLoraArgs a;
        a.a1q = lp; a.a2q = lp + rE; a.a1v = lp + 2 * rE; a.a2v = lp + 3 * rE; a.r = c->d.lora_rank;
        a.pan = panels(c, 0, slot); a.E = c->E; a.ascale = c->ascale; a.layers = c->L; a.st = st; a.f32 = c->f32;
        CHECK(pevit_launch_prep_lora(a, s));
    } else if (post_mlp(c)) {
        const BlockArena& b0 = c->blk[0];
        // (an inference-only context has neither wdT nor wuT: both transposed stores go to its write-only panel, nobody reads them)
        BottleneckPanels bp{at<bf16>(c->arena, b0.wd), at<bf16>(c->arena, c->infer_only ? b0.tsink : b0.wdT), at<bf16>(c->arena, b0.wu),
                            at<bf16>(c->arena, c->infer_only ? b0.tsink : b0.wuT)};
        if (slot >= 0) {        // a slot of a post-MLP slot context (inference-only): its own down and up panels, the same write-only sink
            bp.wd = at<bf16>(c->arena, b0.wds + (size_t)slot * pm_slot_bytes(c));
            bp.wu = at<bf16>(c->arena, b0.wus + (size_t)slot * pm_slot_bytes(c));
        }
        if (c->d.method == PEVIT_ADAPTER) {
            CHECK(pevit_launch_prep_adapter(lp + c->o_dw, lp + c->o_uw, bp, c->E, c->L, st, s, c->f32));
        } else {
            PrepCompacterArgs a;
            a.rule = slot >= 0 ? phm_rule : at<float>(c->arena, c->a_phm); a.dWl = lp + c->o_dWl; a.dWr = lp + c->o_dWr; a.uWl = lp + c->o_uWl; a.uWr = lp + c->o_uWr;
            a.pan = bp; a.E = c->E; a.layers = c->L; a.st = st; a.f32 = c->f32;
            CHECK(pevit_launch_prep_compacter(a, s));
        }
    }
    return 0;
}

// The attention half of block l between ln_1 and out_proj (MultiheadAttention.forward, model.py:612-812): the QKV product with the
// adapter columns t of the attention-site methods, delta-add and the attention core.  Reads the layer's xn1 (or its e4m3 copy a8),
// leaves q / k / v in the head layout, lse and attn_out in the layer's saved slots.  Shared by the block walk and the attention seam.
// Inference walk (pl.infer): the forms without the q' / v' write-back and without lse (f32 verification mode: the saving kernels, on
// the shared slots).
// A multi-slot context (pevit_infer_create_slots: attention-site method, bf16, inference walk) runs the segmented forms throughout.
// Segmented call: the QKV product carries the 64 t columns of EVERY slot, and each segment takes its slot's columns, Q panel and bias.
// Single-adapter call: one segment over the whole batch on the panels behind the last slot -- the product is 64 columns wider still,
// and q, k, v and t keep their bits (the tile families QKV runs on are bit-identical whatever N).
static int attn_core_fwd_slots(pevit_ctx* c, hipStream_t s, int B, const StepPlan& pl, int l) {
    const int E = c->E, T = B * c->N, H = c->H, N = c->N;
    char* W = c->ws; char* A = c->arena;
    const BlockArena& b = c->blk[l];
    const LayerSaved& v = c->lay.sav[l];
    bf16* qkv = at<bf16>(W, v.qkv);
    const size_t plane = (size_t)T * E;
    const int tcols = 64 * (pl.segments ? c->slots : c->slots + 1);
    {
        GemmParams p = gp(at<bf16>(W, v.xn1), E, at<bf16>(A, b.wqkv), E, c->NQpad, T, 3 * E + tcols, E);
        p.bias = at<float>(A, b.bqkv); p.outb = qkv; p.head_stride = plane; p.outf = at<float>(W, v.t); p.ldo = tcols;
        p.E = E; p.H = H; p.Ntok = N;
        CHECK(gemm(c, EPI_QKV_HEADS, p, s));
    }
    const bool kad = c->d.method == PEVIT_KADAPTATION;
    const size_t boff = c->p_layer0 + c->p_layer_stride * l + 4 * (size_t)E;      // the delta bias of layer l in a flat buffer
    AttnSiteSegArgs a;
    a.q = qkv; a.k = qkv + plane; a.v = qkv + 2 * plane; a.t = at<float>(W, v.t); a.tpitch = tcols; a.ascale = c->ascale;
    a.out = at<bf16>(W, v.attn_out); a.ldo = E; a.B = B; a.H = H; a.N = N;
    if (pl.segments) {
        a.nseg = c->nseg;
        for (int i = 0; i < c->nseg; ++i) {
            const pevit_segment& g = c->segs[i];
            a.seg[i].first = g.first; a.seg[i].count = g.count; a.seg[i].tcol = 64 * g.slot;
            a.seg[i].q16 = at<bf16>(A, b.q16s + (size_t)g.slot * q16_slot_bytes(c));
            a.seg[i].bias = kad ? c->slot_params[g.slot] + boff : nullptr;
        }
    } else {
        a.nseg = 1;
        a.seg[0].first = 0; a.seg[0].count = B; a.seg[0].tcol = 64 * c->slots; a.seg[0].q16 = at<bf16>(A, b.q16);
        a.seg[0].bias = kad ? c->params + boff : nullptr;
    }
    if (pl.attn_delta) {
        PROF(c, s, PEVIT_PROF_ATTN_FWD_DELTA, T, (double)T * E * 4 * 2 + (double)T * 64 * 4, pevit_launch_attn_fwd_delta_seg(a, s));
        return 0;
    }
    PROF(c, s, PEVIT_PROF_DELTA_ADD, T, (double)T * E * 4 * c->es + (double)T * 64 * 4, pevit_launch_delta_add_seg(a, s));
    AttnArgs aa = attn_args(c, B, l);
    aa.lse = nullptr;
    PROF(c, s, PEVIT_PROF_ATTN_FWD, T, (double)T * E * 4 * 2, pevit_launch_attn_fwd(aa, s));
    return 0;
}

int attn_core_fwd(pevit_ctx* c, hipStream_t s, int B, const StepPlan& pl, int l, unsigned char* a8, unsigned char* attn8) {
    const int E = c->E, T = B * c->N, H = c->H, N = c->N;
    char* W = c->ws; char* A = c->arena;
    const bool site = pl.site;
    const BlockArena& b = c->blk[l];
    const LayerSaved& v = c->lay.sav[l];
    bf16* qkv = at<bf16>(W, v.qkv);
    const size_t plane = (size_t)T * E;
    if (site_slots(c)) return attn_core_fwd_slots(c, s, B, pl, l);
    if (!c->fp8) {
        GemmParams p = gp(at<bf16>(W, v.xn1), E, at<bf16>(A, b.wqkv), E, c->NQpad, T, site ? c->NQ : 3 * E, E);
        p.bias = at<float>(A, b.bqkv); p.outb = qkv; p.head_stride = plane; p.outf = at<float>(W, v.t); p.ldo = 64;
        p.E = E; p.H = H; p.Ntok = N;
        CHECK(gemm(c, EPI_QKV_HEADS, p, s));
    } else {
        // fp8 codes for the 3E frozen rows; the 64 trainable adapter rows stay bf16: as the bf16 tail of the same launch where the
        // product runs on the staggered 8-wave kernel (round 4: the separate t = xn P product was the whole 1-2 % by which
        // the fp8 format trailed bf16), as a small product of their own otherwise
        GemmParams p = gpw(c, at<bf16>(W, v.xn1), E, b.wqkv, E, 3 * E, T, 3 * E, E, b.sqkv);
        if (a8) { p.A = reinterpret_cast<const bf16*>(a8); p.a_fp8 = 1; }
        p.bias = at<float>(A, b.bqkv); p.outb = qkv; p.head_stride = plane; p.E = E; p.H = H; p.Ntok = N;
        bool tail = false;
        if (pl.fp8_tail) {
            GemmParams m = p;
            m.N = c->NQ; m.B2 = at<bf16>(A, b.wpan); m.ldb2 = E; m.Nb2 = 128; m.n_fp8 = 3 * E; m.outf = at<float>(W, v.t); m.ldo = 64;
            if (pevit_gemm_mixed_ok(m, c->tune)) { p = m; tail = true; }
        }
        CHECK(gemm(c, EPI_QKV_HEADS, p, s));
        if (site && !tail) {
            GemmParams q = gp(at<bf16>(W, v.xn1), E, at<bf16>(A, b.wpan), E, 128, T, 64, E);
            q.outf = at<float>(W, v.t); q.ldo = 64;
            CHECK(gemm(c, EPI_F32, q, s));
        }
    }
    const float* dbias = nullptr;
    if (c->d.method == PEVIT_KADAPTATION) dbias = c->params + c->p_layer0 + c->p_layer_stride * l + 4 * (size_t)E;
    if (pl.attn_delta) {
        AttnFwdDeltaArgs a;
        a.q = qkv; a.k = qkv + plane; a.v = qkv + 2 * plane; a.t = at<float>(W, v.t); a.q16 = at<bf16>(A, b.q16); a.bias = dbias;
        a.ascale = c->ascale; a.out = at<bf16>(W, v.attn_out); a.ldo = E; a.lse = at<float>(W, v.lse); a.B = B; a.H = H; a.N = N;
        if (pl.infer) { a.nosave = 1; a.lse = nullptr; }
        PROF(c, s, PEVIT_PROF_ATTN_FWD_DELTA, T,       // q, k, v in; q', v', out (inference: out only) and lse
             (double)T * E * (3 + (pl.infer ? 0 : 2) + 1) * 2 + (double)T * 64 * 4 + (pl.infer ? 0.0 : (double)B * H * N * 4),
             pevit_launch_attn_fwd_delta(a, s));
    } else {
        if (site) {
            DeltaAddArgs a;
            a.qbuf = qkv; a.vbuf = eadv(c, qkv, 2 * plane); a.t = at<float>(W, v.t); a.q32 = at<float>(A, b.q32); a.q16 = at<bf16>(A, b.q16);
            a.bias = dbias; a.ascale = c->ascale; a.B = B; a.N = N; a.E = E; a.f32 = c->f32;
            PROF(c, s, PEVIT_PROF_DELTA_ADD, T, (double)T * E * 4 * c->es + (double)T * 64 * 4,     // q and v read + written, t read
                 pevit_launch_delta_add(a, s));
        }
        AttnArgs a = attn_args(c, B, l);
        a.out_fp8 = attn8;
        if (c->causal) {        // the text tower (attn_causal.hip): q, k, v in, out written, nothing else
            if (c->f32) CHECK(pevit_launch_attn_fwd_causal_f32(a, s));
            else PROF(c, s, PEVIT_PROF_ATTN_FWD, T, (double)T * E * 4 * 2, pevit_launch_attn_fwd_causal(a, s));
        } else if (c->f32) {
            CHECK(pevit_launch_attn_fwd_f32(a, s));
        } else {
            if (pl.infer) a.lse = nullptr;
            PROF(c, s, PEVIT_PROF_ATTN_FWD, T, (double)T * E * 4 * 2 + (pl.infer ? 0.0 : (double)B * H * N * 4), pevit_launch_attn_fwd(a, s));
        }
    }
    return 0;
}

// The post-MLP adapter of block l in a segmented call (pevit_predict_segments on a post-MLP slot context): c_proj runs once on all
// rows, the adapter per segment on the panels of the segment's slot and the f32 vectors of the slot's flat buffer.
//   fused route:   ONE adapter_fwd_seg launch, whose workgroups never cross a segment end;
//   unfused route: LayerNorm, down and up product per segment on its row range -- the launches pevit_predict makes for those rows alone.
static int post_mlp_fwd_segments(pevit_ctx* c, hipStream_t s, int B, const StepPlan& pl, int l, const float* x_mid, float* x_out) {
    const int E = c->E, N = c->N, T = B * N;
    char* W = c->ws; char* A = c->arena;
    const BlockArena& b = c->blk[l];
    const LayerSaved& v = c->lay.sav[l];
    const size_t poff = c->p_layer0 + c->p_layer_stride * l;           // layer l's parameters in a flat buffer
    auto wd_of = [&](int slot) { return at<bf16>(A, b.wds + (size_t)slot * pm_slot_bytes(c)); };
    auto wu_of = [&](int slot) { return at<bf16>(A, b.wus + (size_t)slot * pm_slot_bytes(c)); };
    if (pl.adapter_fused) {
        GemmParams p = gp(at<bf16>(W, c->lay.w_g), 4 * E, at<bf16>(A, b.wpr), 4 * E, E, T, E, 4 * E);
        p.outf = at<float>(W, v.hf32); p.ldo = E;
        CHECK(gemm(c, EPI_F32, p, s));
        AdapterFwdSegArgs a;
        a.act_kind = act_kind(c); a.hraw = at<float>(W, v.hf32); a.bpr = at<float>(A, b.bpr); a.x_mid = x_mid; a.x_out = x_out; a.E = E;
        a.nseg = c->nseg;
        for (int i = 0; i < c->nseg; ++i) {
            const pevit_segment& g = c->segs[i];
            const float* lp = c->slot_params[g.slot] + poff;
            AdapterSegment& o = a.seg[i];
            o.first = g.first * N; o.end = (g.first + g.count) * N;
            o.gamma = lp + c->o_nw; o.beta = lp + c->o_nb; o.wd = wd_of(g.slot); o.b_down = lp + c->o_db; o.wu = wu_of(g.slot); o.b_up = lp + c->o_ub;
        }
        PROF(c, s, PEVIT_PROF_ADAPTER_FWD, T, (double)T * E * (4 + 4 + 4) + (double)c->nseg * 2 * 64 * E * 2, pevit_launch_adapter_fwd_seg(a, s));
        return 0;
    }
    float* ytmp = at<float>(W, c->lay.w_dxn);           // x_mid + h
    {
        GemmParams p = gp(at<bf16>(W, c->lay.w_g), 4 * E, at<bf16>(A, b.wpr), 4 * E, E, T, E, 4 * E);
        p.bias = at<float>(A, b.bpr); p.resid = x_mid; p.ldr = E; p.outf = ytmp; p.ldo = E;
        p.outf2 = at<float>(W, v.hf32); p.ldo2 = E;
        CHECK(gemm(c, EPI_BIAS_RESID_KEEP, p, s));
    }
    for (int i = 0; i < c->nseg; ++i) {
        const pevit_segment& g = c->segs[i];
        const float* lp = c->slot_params[g.slot] + poff;
        const size_t r0 = (size_t)g.first * N;
        const int Ts = g.count * N;
        bf16* z = at<bf16>(W, v.z) + r0 * E;
        bf16* act = at<bf16>(W, v.act) + r0 * 64;
        {
            LnFwdArgs a;
            a.x = at<float>(W, v.hf32) + r0 * E; a.gamma = lp + c->o_nw; a.beta = lp + c->o_nb; a.rows = Ts; a.E = E; a.y_bf16 = z;
            CHECK(pevit_launch_ln_fwd(a, s));
        }
        {
            GemmParams p = gp(z, E, wd_of(g.slot), E, 64, Ts, 64, E);
            p.bias = lp + c->o_db;
            if (c->d.method == PEVIT_ADAPTER) {
                p.outb = act; p.ldob = 64;
                CHECK(gemm(c, EPI_BIAS_RELU_BF16, p, s));
            } else {
                p.outb = at<bf16>(W, v.apre) + r0 * 64; p.ldob = 64; p.outb2 = act; p.ldob2 = 64;
                CHECK(gemm(c, EPI_BIAS_GELUNEW, p, s));
            }
        }
        {
            GemmParams p = gp(act, 64, wu_of(g.slot), 64, E, Ts, E, 64);
            p.bias = lp + c->o_ub; p.resid = ytmp + r0 * E; p.ldr = E; p.outf = x_out + r0 * E; p.ldo = E;
            CHECK(gemm(c, EPI_BIAS_RESID_F32, p, s));
        }
    }
    return 0;
}

// forward of the L residual blocks on internal (batch-major) rows.  x0 -> sav[0].x_in must
// already hold the input; the output lands in ws + w_xfinal.
// cls_only: the caller consumes only the class token of the last block (VisionTransformer.forward,
// model.py:1046) -- everything of the last block that sits after the attention core is then
// evaluated on the B class-token rows only (identical results, ~6 % fewer FLOPs per step).  Never with post-MLP adapters
// (StepPlan::cls_prune).
// Inference walk (pl.infer; the layout must be layout_workspace(.., infer = true)): the same launches in the same order with the
// LayerNorm statistics, lse, q' / v' and the MLP pre-activation h not written; bit-identical x_final.  The post-MLP adapter kernels
// keep writing z / act / apre / mean_a / rstd_a -- into the slots all layers share.
int blocks_forward(pevit_ctx* c, hipStream_t s, int B, const StepPlan& pl, bool cls_only, int l_lo, int l_hi) {
    if (l_hi < 0) l_hi = c->L;
    const int E = c->E, T = B * c->N, N = c->N;
    char* W = c->ws; char* A = c->arena;
    if ((pl.site || pl.post_mlp) && !pl.segments) CHECK(prep_adapters(c, s));     // (a segmented call reads the panels its slots were loaded with)
    for (int l = l_lo; l < l_hi; ++l) {
        const BlockArena& b = c->blk[l];
        const LayerSaved& v = c->lay.sav[l];
        float* x_in = at<float>(W, v.x_in);
        float* x_mid = at<float>(W, v.x_mid);
        float* x_out = (l + 1 < c->L) ? at<float>(W, c->lay.sav[l + 1].x_in) : at<float>(W, c->lay.w_xfinal);
        // x = x + attn(ln_1(x))                                         model.py:973
        unsigned char* a8 = c->fp8act ? at<unsigned char>(W, c->lay.w_a8) : nullptr;
        unsigned char* attn8 = c->fp8act ? at<unsigned char>(W, c->lay.w_attn8) : nullptr;
        {
            LnFwdArgs a;
            a.x = x_in; a.gamma = at<float>(A, b.ln1w); a.beta = at<float>(A, b.ln1b); a.rows = T; a.E = E; a.y_bf16 = at<bf16>(W, v.xn1);
            if (!pl.infer) { a.mean = at<float>(W, v.mean1); a.rstd = at<float>(W, v.rstd1); }
            a.f32 = c->f32; a.y_fp8 = a8;
            PROF(c, s, PEVIT_PROF_LN_FWD, T, (double)T * E * (4 + c->es), pevit_launch_ln_fwd(a, s));
        }
        CHECK(attn_core_fwd(c, s, B, pl, l, a8, attn8));
        // rows of the tail of this block: all T, or (last block, cls_only) the B class-token rows, which
        // sit N*E elements apart in every [T][E] buffer
        const bool cls = cls_only && l == c->L - 1;
        const int R = cls ? B : T;
        const int rs = cls ? N * E : E;            // row stride of [T][E] buffers
        {
            GemmParams p = gpw(c, at<bf16>(W, v.attn_out), rs, b.wo, E, E, R, E, E, b.so);
            if (attn8) { p.A = reinterpret_cast<const bf16*>(attn8); p.a_fp8 = 1; }
            p.bias = at<float>(A, b.bo); p.resid = x_in; p.ldr = rs; p.outf = x_mid; p.ldo = rs;
            CHECK(gemm(c, EPI_BIAS_RESID_F32, p, s));
        }
        // x = x + mlp(ln_2(x))                                          model.py:974
        {
            LnFwdArgs a;
            a.x = x_mid; a.gamma = at<float>(A, b.ln2w); a.beta = at<float>(A, b.ln2b); a.rows = R; a.E = E; a.y_bf16 = at<bf16>(W, c->lay.w_xn2);
            if (!pl.infer) { a.mean = at<float>(W, v.mean2); a.rstd = at<float>(W, v.rstd2); }
            a.xstride = (size_t)rs; a.f32 = c->f32; a.y_fp8 = a8;
            PROF(c, s, PEVIT_PROF_LN_FWD, R, (double)R * E * (4 + c->es), pevit_launch_ln_fwd(a, s));
        }
        {
            GemmParams p = gpw(c, at<bf16>(W, c->lay.w_xn2), E, b.wfc, E, 4 * E, R, 4 * E, E, b.sfc);
            if (a8) { p.A = reinterpret_cast<const bf16*>(a8); p.a_fp8 = 1; p.out2_fp8 = 1; }     // gelu(h) leaves as e4m3 codes
            p.bias = at<float>(A, b.bfc); p.outb2 = at<bf16>(W, c->lay.w_g); p.ldob2 = 4 * E;
            if (!pl.infer) { p.outb = at<bf16>(W, v.h); p.ldob = 4 * E; }
            CHECK(gemm(c, pl.infer ? EPI_BIAS_GELU_ONLY : EPI_BIAS_GELU, p, s));
        }
        if (!pl.post_mlp) {
            GemmParams p = gpw(c, at<bf16>(W, c->lay.w_g), 4 * E, b.wpr, 4 * E, E, R, E, 4 * E, b.spr);
            if (a8) p.a_fp8 = 1;
            p.bias = at<float>(A, b.bpr); p.resid = x_mid; p.ldr = rs; p.outf = x_out; p.ldo = rs;
            CHECK(gemm(c, EPI_BIAS_RESID_F32, p, s));
            continue;
        }
        // x = x + [h + up(act(down(LN_a(h))))]         adapter_model.py:330-336 / compacter_model.py:497-503
        if (pl.segments) {          // (no adapter need be selected: every operand comes from the segments' slots)
            CHECK(post_mlp_fwd_segments(c, s, B, pl, l, x_mid, x_out));
            continue;
        }
        const float* lp = c->params + c->p_layer0 + c->p_layer_stride * l;
        if (pl.adapter_fused) {
            // two launches (adapter_fused.hip): c_proj writes its accumulators once (the bias joins in the adapter kernel), then
            // LayerNorm -> down -> activation -> up -> residual for 32 rows per workgroup
            GemmParams p = gp(at<bf16>(W, c->lay.w_g), 4 * E, at<bf16>(A, b.wpr), 4 * E, E, T, E, 4 * E);
            p.outf = at<float>(W, v.hf32); p.ldo = E;
            CHECK(gemm(c, EPI_F32, p, s));
            AdapterFwdArgs a;
            a.act_kind = act_kind(c); a.hraw = at<float>(W, v.hf32); a.bpr = at<float>(A, b.bpr); a.x_mid = x_mid;
            a.gamma = lp + c->o_nw; a.beta = lp + c->o_nb; a.wd = at<bf16>(A, b.wd); a.b_down = lp + c->o_db; a.wu = at<bf16>(A, b.wu);
            a.b_up = lp + c->o_ub; a.z = at<bf16>(W, v.z); a.mean_a = at<float>(W, v.mean_a); a.rstd_a = at<float>(W, v.rstd_a);
            a.act = at<bf16>(W, v.act); a.apre = at<bf16>(W, v.apre); a.x_out = x_out; a.T = T; a.E = E;
            PROF(c, s, PEVIT_PROF_ADAPTER_FWD, T, (double)T * E * (4 + 4 + 4 + 2) + (double)T * 64 * 4, pevit_launch_adapter_fwd(a, s));
            continue;
        }
        float* ytmp = at<float>(W, c->lay.w_dxn);           // x_mid + h ; scratch that is free during the forward pass
        {
            GemmParams p = gp(at<bf16>(W, c->lay.w_g), 4 * E, at<bf16>(A, b.wpr), 4 * E, E, T, E, 4 * E);
            p.bias = at<float>(A, b.bpr); p.resid = x_mid; p.ldr = E; p.outf = ytmp; p.ldo = E;
            p.outf2 = at<float>(W, v.hf32); p.ldo2 = E;
            CHECK(gemm(c, EPI_BIAS_RESID_KEEP, p, s));
        }
        {
            LnFwdArgs a;
            a.x = at<float>(W, v.hf32); a.gamma = lp + c->o_nw; a.beta = lp + c->o_nb; a.rows = T; a.E = E; a.y_bf16 = at<bf16>(W, v.z);
            if (!pl.infer) { a.mean = at<float>(W, v.mean_a); a.rstd = at<float>(W, v.rstd_a); }
            a.f32 = c->f32;
            CHECK(pevit_launch_ln_fwd(a, s));
        }
        {
            GemmParams p = gp(at<bf16>(W, v.z), E, at<bf16>(A, b.wd), E, 64, T, 64, E);
            p.bias = lp + c->o_db;
            if (c->d.method == PEVIT_ADAPTER) {
                p.outb = at<bf16>(W, v.act); p.ldob = 64;
                CHECK(gemm(c, EPI_BIAS_RELU_BF16, p, s));
            } else {
                p.outb = at<bf16>(W, v.apre); p.ldob = 64; p.outb2 = at<bf16>(W, v.act); p.ldob2 = 64;
                CHECK(gemm(c, EPI_BIAS_GELUNEW, p, s));
            }
        }
        {
            GemmParams p = gp(at<bf16>(W, v.act), 64, at<bf16>(A, b.wu), 64, E, T, E, 64);
            p.bias = lp + c->o_ub; p.resid = ytmp; p.ldr = E; p.outf = x_out; p.ldo = E;
            CHECK(gemm(c, EPI_BIAS_RESID_F32, p, s));
        }
    }
    return 0;
}

// The attention half of block l's backward (the autograd of model.py:612-812 without the QKV dX product): ws+w_dyb (bf16, fp8: with
// out_proj's channel scales folded in) -> out_proj dX -> attention backward into dqkv -> the low-rank adapter gradient partials of
// the attention-site methods.  cls: class-token pruning of the last block (only the B class-token rows of dyb are defined).
int attn_core_bwd(pevit_ctx* c, hipStream_t s, int B, const StepPlan& pl, int l, bool cls, AttnGradWalk& w) {
    const int E = c->E, T = B * c->N, H = c->H, N = c->N;
    char* W = c->ws; char* A = c->arena;
    const int chunks = pevit_lowrank_chunks(T);
    const BlockArena& b = c->blk[l];
    const LayerSaved& v = c->lay.sav[l];
    bf16* dqkv = at<bf16>(W, c->lay.w_dqkv);
    bf16* dyb = at<bf16>(W, c->lay.w_dyb);
    const int R = cls ? B : T;
    const int rs = cls ? N * E : E;            // row stride of [T][E] buffers
    {
        GemmParams p = gpw(c, dyb, rs, b.woT, E, E, R, E, E, 0);
        p.outb = at<bf16>(W, c->lay.w_dO); p.ldob = rs;
        CHECK(gemm(c, EPI_BF16, p, s));
    }
    {
        AttnArgs a = attn_args(c, B, l);
        a.dout = at<bf16>(W, c->lay.w_dO); a.lddo = E; a.dqkv = dqkv; a.ld = c->NQ; a.dout_cls_only = (cls && N <= 64) ? 1 : 0;
        if (c->f32)
            CHECK(pevit_launch_attn_bwd_f32(a, s));
        else
            PROF(c, s, PEVIT_PROF_ATTN_BWD, T, (double)T * E * (N <= 64 ? 7 : 8) * 2 + (double)B * H * N * 4,     // q, k, v, (out: N > 64 only), dout in; dq, dk, dv out
                 pevit_launch_attn_bwd(a, s));
    }
    if (!pl.site) return 0;
    // the low-rank adapter gradients: u (f32, and bf16 into the 64 adapter columns of dqkv), dQ / d bias and dP partials of this layer
    LowrankArgs a;
    a.dqkv = dqkv; a.ld = c->NQ; a.qT = at<bf16>(A, b.qT); a.q32 = at<float>(A, b.q32); a.u_bf16_cols = eadv(c, dqkv, 3 * (size_t)E);
    a.t = at<float>(W, v.t); a.ldx = E; a.B = B; a.H = H; a.N = N; a.E = E;
    a.partial = at<float>(W, c->lay.w_partial + (size_t)l * c->lay.partial_layer);
    a.dbias_partial = at<float>(W, c->lay.w_dbias + (size_t)l * c->lay.dbias_layer);
    if (pl.lowrank_combo) {
        // u, dQ_q, dQ_v, d bias of this layer and the dP of the layer before it in ONE launch (lowrank.hip lowrank_combo_kernel)
        a.this_layer = 1; a.u32 = at<float>(W, w.u_par ? c->lay.w_u32b : c->lay.w_u32);
        if (w.prev_layer >= 0) {
            a.prev = 1; a.xn_prev = at<bf16>(W, c->lay.sav[w.prev_layer].xn1); a.u32_prev = w.u_last;
            a.partial_prev = at<float>(W, c->lay.w_partial + (size_t)w.prev_layer * c->lay.partial_layer);
        }
        PROF(c, s, PEVIT_PROF_LOWRANK_BWD, T, (double)T * E * 3 * 2 + (double)T * 64 * 14 + (double)chunks * 4 * E * 32 * 4,
             pevit_launch_lowrank_combo(a, s));
        w.u_last = a.u32; w.prev_layer = l; w.u_par ^= 1;
    } else {
        a.u32 = at<float>(W, c->lay.w_u32); a.xn = at<bf16>(W, v.xn1); a.chunks = chunks; a.xcd_order = pl.lowrank_xcd;
        if (c->f32) {
            CHECK(pevit_launch_lowrank_u_f32(a, s));
            CHECK(pevit_launch_lowrank_grad_f32(a, s));
        } else {
            PROF(c, s, PEVIT_PROF_LOWRANK_U, T, (double)T * E * 2 * 2 + (double)T * 64 * 6, pevit_launch_lowrank_u(a, s));
            PROF(c, s, PEVIT_PROF_LOWRANK_GRAD, T, (double)T * E * 3 * 2 + (double)T * 64 * 8 + (double)chunks * 4 * E * 32 * 4,
                 pevit_launch_lowrank_grad(a, s));
        }
    }
    return 0;
}

// QKV dX of block l: dqkv (incl. the 64 adapter columns u of the attention-site methods) -> the gradient of the attention input.
// dx_f32 == nullptr: into ws+w_dxn in the block walk's hand-over type (bf16 with dx_stored, for LayerNorm backward); else f32 [T][E].
int attn_qkv_dx(pevit_ctx* c, hipStream_t s, int B, const StepPlan& pl, int l, float* dx_f32) {
    const int E = c->E, T = B * c->N;
    float* dxn = at<float>(c->ws, c->lay.w_dxn);
    GemmParams p = gp(at<bf16>(c->ws, c->lay.w_dqkv), c->NQ, at<bf16>(c->arena, c->blk[l].wqkvT), c->NQ, E, T, E, pl.site ? c->NQ : 3 * E);
    if (dx_f32) { p.outf = dx_f32; p.ldo = E; CHECK(gemm(c, EPI_F32, p, s)); }
    else if (pl.dx_stored) { p.outb = reinterpret_cast<bf16*>(dxn); p.ldob = E; CHECK(gemm(c, EPI_BF16, p, s)); }
    else { p.outf = dxn; p.ldo = E; CHECK(gemm(c, EPI_F32, p, s)); }
    return 0;
}

// end of a walk: the deferred dP of the last layer walked (lowrank_combo)
int attn_walk_end(pevit_ctx* c, hipStream_t s, int B, AttnGradWalk& w) {
    const int E = c->E, T = B * c->N, H = c->H, N = c->N;
    if (w.prev_layer >= 0) {
        LowrankArgs a;      // this_layer stays 0: only the "previous layer" operands are read
        a.prev = 1; a.xn_prev = at<bf16>(c->ws, c->lay.sav[w.prev_layer].xn1); a.ldx = E; a.u32_prev = w.u_last;
        a.partial_prev = at<float>(c->ws, c->lay.w_partial + (size_t)w.prev_layer * c->lay.partial_layer);
        a.B = B; a.H = H; a.N = N; a.E = E;
        PROF(c, s, PEVIT_PROF_LOWRANK_BWD, T, (double)T * E * 2 + (double)T * 64 * 4, pevit_launch_lowrank_combo(a, s));
    }
    w.prev_layer = -1;
    return 0;
}

// post-MLP adapters: a token-contracted weight-gradient product G = X^T Y of layer l into its per-chunk partials (X: [T][E], Y: [T][64])
static int tn_product(pevit_ctx* c, hipStream_t s, int T, const bf16* X, const bf16* Y, size_t w_partial, int l, bool csy) {
    TnGemm64Args a;
    a.X = X; a.ldx = c->E; a.Y = Y; a.ldy = 64; a.partial = at<float>(c->ws, w_partial + (size_t)l * c->lay.tn_layer);
    if (csy) a.csy = at<float>(c->ws, c->lay.w_csy + (size_t)l * c->lay.csy_layer);
    a.T = T; a.E = c->E;
    return c->f32 ? pevit_launch_tn_gemm64_f32(a, s) : pevit_launch_tn_gemm64(a, s);
}

// adapter gradients of layers [l_lo, l_hi): reduce the per-layer partials and chain onto the reference's tensors (flat gradient
// buffer, accumulating)
int reduce_adapter_grads(pevit_ctx* c, hipStream_t s, int B, const StepPlan& pl, int l_lo, int l_hi) {
    const int E = c->E, T = B * c->N;
    char* W = c->ws;
    const int chunks = pevit_lowrank_chunks(T);
    const int nl = l_hi - l_lo;
    const size_t pl0 = c->p_layer0 + c->p_layer_stride * l_lo;          // first float of layer l_lo's parameters
    if (nl <= 0) return 0;
    if (c->d.method == PEVIT_KADAPTATION) {
        ChainKadaptArgs a;
        a.partial = at<float>(W, c->lay.w_partial + (size_t)l_lo * c->lay.partial_layer); a.partial_layer = c->lay.partial_layer / 4;
        a.dbias_partial = at<float>(W, c->lay.w_dbias + (size_t)l_lo * c->lay.dbias_layer); a.dbias_layer = c->lay.dbias_layer / 4;
        a.chunks = chunks; a.ascale = c->ascale; a.layers = nl; a.G = at<float>(W, c->lay.w_G) + (size_t)l_lo * 4 * E * 32;
        a.rule_scratch = at<float>(W, c->lay.w_rule) + (size_t)l_lo * 4096; a.params = c->params; a.grads = c->grads;
        a.p_layer0 = pl0; a.p_layer_stride = c->p_layer_stride; a.E = E;
        CHECK(pevit_launch_chain_kadapt(a, s));
        // the shared rule factors collect from every layer: each range adds its own layers (top first, one running sum), so a
        // backward that never reaches block 0 keeps its rule contributions and a walk in ranges equals the one-call backward
        CHECK(pevit_launch_rule_sum(at<float>(W, c->lay.w_rule), c->grads, l_lo, l_hi, s));
    } else if (c->d.method == PEVIT_LORA) {
        ChainLoraArgs a;
        a.partial = at<float>(W, c->lay.w_partial + (size_t)l_lo * c->lay.partial_layer); a.partial_layer = c->lay.partial_layer / 4;
        a.chunks = chunks; a.ascale = c->ascale; a.r = c->d.lora_rank; a.layers = nl; a.G = at<float>(W, c->lay.w_G) + (size_t)l_lo * 4 * E * 32;
        a.grads = c->grads; a.p_layer0 = pl0; a.p_layer_stride = c->p_layer_stride; a.E = E;
        CHECK(pevit_launch_chain_lora(a, s));
    } else if (pl.post_mlp) {
        const int tch = pevit_tn_chunks(T), lnb = pl.adapter_fused ? pevit_adapter_blocks(T) : pevit_lna_blocks(T);
        const size_t ps = c->p_layer_stride, gl = (size_t)E * 64;
        float* g0 = c->grads + pl0;
        float* Gd = at<float>(W, c->lay.w_Gd) + (size_t)l_lo * gl;
        float* Gu = at<float>(W, c->lay.w_Gu) + (size_t)l_lo * gl;
        CHECK(pevit_launch_zero(Gd, (size_t)nl * gl * 4, s));
        CHECK(pevit_launch_zero(Gu, (size_t)nl * gl * 4, s));
        CHECK(pevit_launch_colsum_reduce(at<float>(W, c->lay.w_tnD + (size_t)l_lo * c->lay.tn_layer), tch, (int)gl, Gd, nl, c->lay.tn_layer / 4, gl, s));
        CHECK(pevit_launch_colsum_reduce(at<float>(W, c->lay.w_tnU + (size_t)l_lo * c->lay.tn_layer), tch, (int)gl, Gu, nl, c->lay.tn_layer / 4, gl, s));
        // biases and LayerNorm affine: straight column sums into the flat gradient buffer
        // d b_up from the f32 column sums of the upstream gradient (third plane of the LN partials)
        CHECK(pevit_launch_colsum_reduce(at<float>(W, c->lay.w_csy + (size_t)l_lo * c->lay.csy_layer), tch, 64, g0 + c->o_db, nl,
                                         c->lay.csy_layer / 4, ps, s));
        {
            ColsumReduce3Args a;
            a.partial = at<float>(W, c->lay.w_lnp + (size_t)l_lo * c->lay.lnp_layer); a.chunks = lnb; a.n = E;
            a.o0 = g0 + c->o_nw; a.o1 = g0 + c->o_nb; a.o2 = g0 + c->o_ub; a.layers = nl; a.partial_layer = c->lay.lnp_layer / 4; a.out_layer = ps;
            CHECK(pevit_launch_colsum_reduce3(a, s));
        }
        if (c->d.method == PEVIT_ADAPTER) {
            CHECK(pevit_launch_chain_adapter(Gd, Gu, g0 + c->o_dw, g0 + c->o_uw, E, nl, gl, ps, s));
        } else {
            ChainCompacterArgs a;
            a.Gd = Gd; a.Gu = Gu; a.rule = at<float>(c->arena, c->a_phm); a.params = c->params + pl0; a.grads = g0; a.E = E; a.layers = nl;
            a.g_layer = gl; a.param_layer = ps; a.off_dWl = c->o_dWl; a.off_dWr = c->o_dWr; a.off_uWl = c->o_uWl; a.off_uWr = c->o_uWr;
            CHECK(pevit_launch_chain_compacter(a, s));
        }
    }
    return 0;
}

// backward of the blocks.  On entry ws+w_dxa holds dL/dx_final (f32) and ws+w_dyb its bf16 copy (StepPlan::gstream16: only
// the bf16 copy is read).
// On exit ws+w_dxa holds dL/dx_0 if need_dx0.
// cls_only mirrors blocks_forward: on entry only the class-token rows of dxa / dyb are defined (and
// read); dxb and dO must have been zeroed by the caller.
// Layers l_hi-1 .. l_lo are processed (the whole tower: L, 0) and the adapter gradients of exactly these layers are
// reduced and chained onto the reference's tensors at the end -- data parallelism runs the tower in two halves so that
// the all-reduce of the upper half's gradients overlaps the backward of the lower half.
int blocks_backward(pevit_ctx* c, hipStream_t s, int B, const StepPlan& pl, bool need_dx0, bool cls_only, int l_hi, int l_lo) {
    const int E = c->E, T = B * c->N, N = c->N;
    char* W = c->ws; char* A = c->arena;
    float* dxa = at<float>(W, c->lay.w_dxa);
    float* dxb = at<float>(W, c->lay.w_dxb);
    bf16* dyb = at<bf16>(W, c->lay.w_dyb);
    float* dxn = at<float>(W, c->lay.w_dxn);
    const bool gs16 = pl.gstream16;
    // bytes LayerNorm backward moves per row element: dy (stored type or f32) + x + residual gradient read, gradient written
    const size_t ln_bwd_bytes = (pl.dx_stored ? c->es : 4) + 4 + (gs16 ? c->es : 4 + 4) + c->es;
    // what both LayerNorm backward launches of every block share: the LN-input gradient of the dX GEMM before them in dxn, the bf16
    // copy of the result (the next dX GEMM's operand) in dyb
    LnBwdArgs ln_bwd_base;
    ln_bwd_base.dy = dxn; ln_bwd_base.dx_bf16 = dyb; ln_bwd_base.E = E; ln_bwd_base.f32 = c->f32; ln_bwd_base.dy_stored = pl.dx_stored;
    ln_bwd_base.res16 = gs16;
    AttnGradWalk walk;
    int tn_pend = -1, tn_par = 0;          // post-MLP adapters: layer whose d W_down product is still owed, and the d pre buffer in turn
    const bf16* tn_pend_dpre = nullptr;
    for (int l = l_hi - 1; l >= l_lo; --l) {
        const BlockArena& b = c->blk[l];
        const LayerSaved& v = c->lay.sav[l];
        const bf16* mlp_dy = dyb;          // upstream gradient of the MLP output (bf16)
        if (pl.post_mlp) {
            // out = x_mid + h + up(act(down(LN_a(h)))) :  dx_out (dxa, dyb) flows to x_mid, to h, and into the adapter
            const float* lp = c->params + c->p_layer0 + c->p_layer_stride * l;
            const bool fold = pl.tn_fold;      // both weight-gradient products inside the backward launch
            bf16* dpre = at<bf16>(W, (fold && tn_par) ? c->lay.w_dpre2 : c->lay.w_dpre);
            // d W_up[e][j] = sum_r dx_out[r][e] act[r][j] ; d b_up = colsum(dx_out)
            if (!fold) CHECK(tn_product(c, s, T, dyb, at<bf16>(W, v.act), c->lay.w_tnU, l, false));
            if (pl.adapter_fused) {
                const int dwl = tn_pend >= 0 ? tn_pend : l;       // the layer whose d W_down product this launch carries (if any)
                // d pre, d z and the LayerNorm backward with its affine-gradient column sums in one launch (adapter_fused.hip); the
                // forward pass left the c_proj accumulators WITHOUT their bias in hf32
                AdapterBwdArgs a;
                a.act_kind = act_kind(c); a.dyb = dyb; a.wuT = at<bf16>(A, b.wuT); a.wdT = at<bf16>(A, b.wdT);
                if (!gs16) a.dres = dxa;
                a.saved = at<bf16>(W, a.act_kind == 0 ? v.act : v.apre);
                a.hraw = at<float>(W, v.hf32); a.bpr = at<float>(A, b.bpr); a.mean_a = at<float>(W, v.mean_a); a.rstd_a = at<float>(W, v.rstd_a);
                a.gamma = lp + c->o_nw; a.dpre = dpre; a.dh_bf16 = at<bf16>(W, c->lay.w_dhb);
                a.partial = at<float>(W, c->lay.w_lnp + (size_t)l * c->lay.lnp_layer); a.T = T; a.E = E;
                if (fold) { a.tn_x1 = dyb; a.tn_y1 = at<bf16>(W, v.act); a.tn_partial1 = at<float>(W, c->lay.w_tnU + (size_t)l * c->lay.tn_layer); }
                if (fold && tn_pend >= 0) {
                    a.tn_x2 = at<bf16>(W, c->lay.sav[dwl].z); a.tn_y2 = tn_pend_dpre;
                    a.tn_partial2 = at<float>(W, c->lay.w_tnD + (size_t)dwl * c->lay.tn_layer);
                    a.tn_csy2 = at<float>(W, c->lay.w_csy + (size_t)dwl * c->lay.csy_layer);
                }
                a.tn_blocks = pl.tn_fold_wgs;
                PROF(c, s, PEVIT_PROF_ADAPTER_BWD, T, (double)T * E * (2 + 4 + 4 + 2) + (double)T * 64 * 4, pevit_launch_adapter_bwd(a, s));
                if (fold) { tn_pend = l; tn_pend_dpre = dpre; tn_par ^= 1; }
            } else {
                {   // d act = dx_out W_up ; d pre = d act * act'(pre)
                    GemmParams p = gp(dyb, E, at<bf16>(A, b.wuT), E, 64, T, 64, E);
                    p.outb = dpre; p.ldob = 64; p.ldaux = 64;
                    if (c->d.method == PEVIT_ADAPTER) { p.aux = at<bf16>(W, v.act); CHECK(gemm(c, EPI_DRELU_BF16, p, s)); }
                    else { p.aux = at<bf16>(W, v.apre); CHECK(gemm(c, EPI_DGELUNEW_BF16, p, s)); }
                }
                {   // d z = d pre W_down
                    GemmParams p = gp(dpre, 64, at<bf16>(A, b.wdT), 64, E, T, E, 64);
                    p.outf = dxn; p.ldo = E;
                    CHECK(gemm(c, EPI_F32, p, s));
                }
            }
            // d W_down[j][e] = sum_r d pre[r][j] z[r][e] ; d b_down = colsum(d pre)
            if (!fold) CHECK(tn_product(c, s, T, at<bf16>(W, v.z), dpre, c->lay.w_tnD, l, true));
            // d h = dx_out + LN_a-backward(d z) ; partial sums for d gamma_a, d beta_a
            if (!pl.adapter_fused) {
                LnBwdAffineArgs a;
                a.dy = dxn; a.x = at<float>(W, v.hf32); a.mean = at<float>(W, v.mean_a); a.rstd = at<float>(W, v.rstd_a); a.gamma = lp + c->o_nw;
                a.dres = dxa; a.dx_bf16 = at<bf16>(W, c->lay.w_dhb); a.partial = at<float>(W, c->lay.w_lnp + (size_t)l * c->lay.lnp_layer);
                a.rows = T; a.E = E; a.f32 = c->f32;
                CHECK(pevit_launch_ln_bwd_affine(a, s));
            }
            mlp_dy = at<bf16>(W, c->lay.w_dhb);
            if (l == 0 && !need_dx0) break;     // nothing trainable below the first block's adapter
        }
        const bool cls = cls_only && l == c->L - 1;
        const int R = cls ? B : T;
        const int rs = cls ? N * E : E;            // row stride of [T][E] buffers
        // ---- MLP branch: d h = (dy W_proj) * gelu'(h) ; d xn2 = d h W_fc
        {
            // fp8: mlp_dy arrives with c_proj's channel scales folded in, and leaves with c_fc's (for the next product)
            GemmParams p = gpw(c, mlp_dy, rs, b.wprT, E, 4 * E, R, 4 * E, E, 0);
            p.aux = at<bf16>(W, v.h); p.ldaux = 4 * E; p.outb = at<bf16>(W, c->lay.w_dh); p.ldob = 4 * E;
            if (c->fp8) p.oscale = at<float>(A, b.sfc);
            CHECK(gemm(c, EPI_DGELU_BF16, p, s));
        }
        {
            // the LN-input gradient leaves the GEMM in the activation storage type (bf16): LayerNorm backward is
            // HBM-bound, and this halves the bytes on both sides of the hand-over
            GemmParams p = gpw(c, at<bf16>(W, c->lay.w_dh), 4 * E, b.wfcT, 4 * E, E, R, E, 4 * E, 0);
            if (pl.dx_stored) { p.outb = reinterpret_cast<bf16*>(dxn); p.ldob = E; CHECK(gemm(c, EPI_BF16, p, s)); }
            else { p.outf = dxn; p.ldo = E; CHECK(gemm(c, EPI_F32, p, s)); }
        }
        // fp8: the bf16 copy feeds the out-projection backward, whose contraction runs over out_proj's output channels.
        // gs16: the residual gradient is the bf16 copy dyb itself, read and rewritten in place (no f32 pair dxa / dxb)
        {
            LnBwdArgs a = ln_bwd_base;
            a.x = at<float>(W, v.x_mid); a.mean = at<float>(W, v.mean2); a.rstd = at<float>(W, v.rstd2); a.gamma = at<float>(A, b.ln2w);
            a.dres = gs16 ? reinterpret_cast<const float*>(dyb) : dxa;
            if (!gs16) a.dx_out = dxb;
            a.rows = R; a.xstride = (size_t)rs;
            if (c->fp8) a.bf16_colscale = at<float>(A, b.so);
            if (gs16 && c->fp8) a.res_colscale = at<float>(A, b.spr);
            PROF(c, s, PEVIT_PROF_LN_BWD, R, (double)R * E * ln_bwd_bytes, pevit_launch_ln_bwd(a, s));
        }
        // ---- attention branch
        CHECK(attn_core_bwd(c, s, B, pl, l, cls, walk));
        if (l > 0 || need_dx0) {
            CHECK(attn_qkv_dx(c, s, B, pl, l, nullptr));
            // fp8: this bf16 copy is the upstream gradient of layer l-1's c_proj backward.  gs16: the f32 copy only where the caller
            // asked for dx (the lowest block walked).  Last block, class-token pruning: the residual gradient sits on the class rows only
            LnBwdArgs a = ln_bwd_base;
            a.x = at<float>(W, v.x_in); a.mean = at<float>(W, v.mean1); a.rstd = at<float>(W, v.rstd1); a.gamma = at<float>(A, b.ln1w);
            a.dres = gs16 ? reinterpret_cast<const float*>(dyb) : dxb;
            if (!gs16 || (need_dx0 && l == l_lo)) a.dx_out = dxa;
            a.rows = T;
            if (c->fp8 && l > 0) a.bf16_colscale = at<float>(A, c->blk[l - 1].spr);
            if (cls) a.res_period = N;
            if (gs16 && c->fp8) a.res_colscale = at<float>(A, b.so);
            PROF(c, s, PEVIT_PROF_LN_BWD, T, (double)T * E * ln_bwd_bytes, pevit_launch_ln_bwd(a, s));
        }
    }
    // (the deferred dP belongs to the attention-site methods, the owed d W_down product to the post-MLP ones: at most one of the
    // two below has work)
    CHECK(attn_walk_end(c, s, B, walk));
    if (tn_pend >= 0)                   // the d W_down product of the last adapter walked
        CHECK(tn_product(c, s, T, at<bf16>(W, c->lay.sav[tn_pend].z), tn_pend_dpre, c->lay.w_tnD, tn_pend, true));
    return reduce_adapter_grads(c, s, B, pl, l_lo, l_hi);
}

}  // namespace pevit_host
