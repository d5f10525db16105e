// The context: error text, the layouts of the weight arena and the workspace, the plan of a step, creation, binding, weight loading,
// the knobs, and the guards every entry point starts with.
#include <stdarg.h>
#include <stdio.h>

#include <algorithm>
#include <new>

#include "host_ctx.h"

static thread_local char g_err[512] = "";
extern "C" void pevit_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* pevit_last_error(void) { return g_err; }
extern "C" int pevit_version(void) { return 1; }

namespace pevit_host {

// the launch paths of a step of batch B: a pure function of the context's dims, weight format and knobs, the batch and the CU count
StepPlan plan_step(const pevit_ctx* c, int B, bool infer) {
    StepPlan p;
    p.infer = infer;
    p.site = attention_site(c);
    p.post_mlp = post_mlp(c);
    p.cls_prune = !p.post_mlp;
    // delta-add and the attention core as ONE launch where a run of heads owns whole reference rows of the raw reshape
    // (attn_delta.hip: N <= 64; ViT-B/32), otherwise delta_add + attn_fwd
    // ... unless its one-workgroup-per-CU runs leave between a quarter and three quarters of the chip empty (measured at batch
    // 64: 128 runs for 256 CUs, the two kernels are 0.6 % of the step faster; fused_attn_delta = 2 forces the fused form)
    if (p.site && c->fused_attn_delta && !c->f32 && !c->fp8act) {
        const int hpw = pevit_attn_delta_hpw(B, c->H, c->N);
        const int runs = hpw > 0 ? (B * c->H + hpw - 1) / hpw : 0;
        p.attn_delta = hpw > 0 && (c->fused_attn_delta > 1 || 4 * runs >= 3 * pevit_num_cus() || 4 * runs <= pevit_num_cus());
    }
    p.fp8_tail = p.site && c->fp8 && !c->fp8act && c->fp8_tail;
    p.adapter_fused = p.post_mlp && c->adapter_fused && !c->f32 && pevit_adapter_fused_ok(c->E);
    p.tn_fold = p.adapter_fused && c->adapter_tn_fold;
    p.tn_fold_wgs = p.tn_fold && c->adapter_tn_fold > 1 ? c->adapter_tn_fold : 0;
    p.dx_stored = c->dx_stored;
    // attention-site adapters, and the post-MLP ones on their fused kernels; never the f32 verification mode
    p.gstream16 = c->gstream16 && !c->f32 && p.dx_stored && (p.site || p.adapter_fused);
    p.lowrank_combo = p.site && c->lowrank_combo && !c->f32;
    p.lowrank_xcd = c->lowrank_xcd;
    return p;
}

// infer: the layout of the inference walk -- no layer keeps anything, so ONE set of activation slots serves every layer and the f32
// residual stream alternates between two input buffers (+ x_mid + w_xfinal: four [T][E] buffers whatever the layer count); the
// pre-activation h and the LayerNorm statistics have no slot at all.  Never larger than the training layout of the same batch.
// An inference-only context (pevit_infer_create) has the third layout whatever `infer` says: the inference layout without every
// slot that only a backward, a gradient reduction or a training head touches.  It does not depend on the layer count.
WsLayout layout_workspace(const pevit_ctx* c, int B, bool infer) {
    Carver cv;
    const size_t T = (size_t)B * c->N, E = c->E, es = c->es;
    WsLayout w{};
    if (c->infer_only) infer = true;
    // stream-K hand-off flags (+1 error word) and partial-tile slabs: first, so that their place does not depend on the batch
    w.w_skflag = cv.take(WS_STATE_BYTES);
    w.w_skslab = cv.take((size_t)c->sk_slots * PEVIT_SK_SLAB_FLOATS * 4);
    w.sav.resize(c->L);
    auto carve_layer = [&]() {
        LayerSaved s{};
        s.x_in = cv.take(T * E * 4);
        s.x_mid = cv.take(T * E * 4);
        if (!infer) {
            s.mean1 = cv.take(T * 4); s.rstd1 = cv.take(T * 4);
            s.mean2 = cv.take(T * 4); s.rstd2 = cv.take(T * 4);
        }
        s.xn1 = cv.take(T * E * es);
        s.qkv = cv.take(3 * T * E * es);
        s.t = cv.take(T * 64 * 4 * (site_slots(c) ? site_slots(c) + 1 : 1));      // (multi-slot context: the columns of every slot + the single-adapter calls')
        s.lse = cv.take((size_t)B * c->H * c->N * 4);
        s.attn_out = cv.take(T * E * es);
        if (!infer) s.h = cv.take(T * 4 * E * es);
        if (post_mlp(c)) {
            s.hf32 = cv.take(T * E * 4); s.mean_a = cv.take(T * 4); s.rstd_a = cv.take(T * 4);
            s.z = cv.take(T * E * es); s.apre = cv.take(T * 64 * es); s.act = cv.take(T * 64 * es);
        }
        return s;
    };
    if (infer) {
        const LayerSaved s0 = carve_layer();
        const size_t x_alt = cv.take(T * E * 4);
        for (int l = 0; l < c->L; ++l) { w.sav[l] = s0; if (l & 1) w.sav[l].x_in = x_alt; }
    } else {
        for (LayerSaved& s : w.sav) s = carve_layer();
    }
    const int chunks = pevit_lowrank_chunks((int)T);
    w.w_xfinal = cv.take(T * E * 4);
    w.w_xn2 = cv.take(T * E * es);
    w.w_g = cv.take(T * 4 * E * es);            // (fp8act: holds gelu(h) as e4m3 codes, half of it used)
    if (c->fp8act) {
        w.w_a8 = cv.take(T * E);
        w.w_attn8 = cv.take(T * E);
    }
    const size_t Bz = (size_t)B, D = c->D;
    if (c->infer_only) {
        // the walk's names for its one [T][E] f32 scratch: the stem's xpre, ytmp of the unfused post-MLP path
        w.w_dxn = cv.take(T * E * 4);
        w.w_patches = cv.take(Bz * c->G2 * (size_t)c->Kpatch * es);
        w.w_xpost = cv.take(Bz * E * es);
        w.w_feat = cv.take(Bz * D * 4);
        w.w_ybn = cv.take(Bz * D * 4);
        w.w_bnrstd = cv.take(D * 4);
        w.w_logits = cv.take(Bz * (size_t)c->d.num_classes * 4);     // (the largest head: pevit_set_infer_params moves c->C below it)
        w.total = cv.off;
        return w;
    }
    w.w_dqkv = cv.take(T * (size_t)c->NQ * es);
    w.w_u32 = cv.take(T * 64 * 4);
    w.w_u32b = cv.take(T * 64 * 4);             // second u buffer: dP of a layer is taken one launch later (lowrank_combo)
    w.w_dO = cv.take(T * E * es);
    w.w_dh = cv.take(T * 4 * E * es);
    w.w_dxn = cv.take(T * E * 4);
    w.w_dxa = cv.take(T * E * 4);
    w.w_dxb = cv.take(T * E * 4);
    w.w_dyb = cv.take(T * E * es);
    // adapter-gradient partials of every layer (reduced once per step, after the layer loop)
    w.partial_layer = align_up((size_t)chunks * 4 * E * 32 * 4, 256);
    w.dbias_layer = align_up((size_t)chunks * 2 * E * 4, 256);
    w.w_partial = cv.take(w.partial_layer * c->L);
    w.w_dbias = cv.take(w.dbias_layer * c->L);
    w.w_G = cv.take((size_t)c->L * 4 * E * 32 * 4);
    w.w_rule = cv.take((size_t)c->L * 4096 * 4);
    if (post_mlp(c)) {
        const int tch = pevit_tn_chunks((int)T), lnb = std::max(pevit_lna_blocks((int)T), pevit_adapter_blocks((int)T));
        w.tn_layer = (size_t)tch * E * 64 * 4; w.csx_layer = (size_t)tch * E * 4; w.csy_layer = (size_t)tch * 64 * 4;
        w.lnp_layer = (size_t)lnb * 3 * E * 4;
        w.w_dpre = cv.take(T * 64 * es);
        w.w_dpre2 = cv.take(T * 64 * es);       // d pre alternates: the deferred d W_down product reads the previous one
        w.w_dht = cv.take(T * E * 4);
        w.w_dhb = cv.take(T * E * es);
        w.w_tnU = cv.take(w.tn_layer * c->L);
        w.w_tnD = cv.take(w.tn_layer * c->L);
        w.w_csx = cv.take(w.csx_layer * c->L);
        w.w_csy = cv.take(w.csy_layer * c->L);
        w.w_lnp = cv.take(w.lnp_layer * c->L);
        w.w_Gd = cv.take((size_t)c->L * E * 64 * 4);
        w.w_Gu = cv.take((size_t)c->L * E * 64 * 4);
    }
    const size_t Cc = c->C;
    w.w_patches = cv.take(Bz * c->G2 * (size_t)c->Kpatch * es);
    w.w_xpost = cv.take(Bz * E * es);
    w.w_feat = cv.take(Bz * D * 4);
    w.w_pmean = cv.take(Bz * 4);
    w.w_prstd = cv.take(Bz * 4);
    w.w_ybn = cv.take(Bz * D * 4);
    w.w_bnrstd = cv.take(D * 4);
    w.w_logits = cv.take(Bz * Cc * 4);
    w.w_dlogits = cv.take(Bz * Cc * 4);
    w.w_dybn = cv.take(Bz * D * 4);
    w.w_dfeat = cv.take(Bz * D * 4);
    w.w_dfeatb = cv.take(Bz * D * es);
    w.w_dxpost = cv.take(Bz * E * 4);
    w.total = cv.off;
    return w;
}

// the per-layer weight slots of the arena (c->blk must hold c->L entries): what pevit_load_block fills
// An inference-only context (pevit_infer_create) has no slot for what only a backward reads: wqkvT, woT, wfcT, wprT, wdT, wuT.  The
// prep kernels store the transposed adapter panels whoever runs them, so such a context gives them ONE write-only [E][64] panel per
// layer (tsink) in place of the 64 adapter columns of wqkvT (attention-site methods) or of wdT and wuT (post-MLP methods).
static void carve_block_arena(pevit_ctx* c, Carver& cv) {
    const size_t E = c->E;
    for (int l = 0; l < c->L; ++l) {
        BlockArena& b = c->blk[l];
        b.wpan = b.sqkv = b.so = b.sfc = b.spr = b.tsink = 0;
        if (c->infer_only) {
            if (c->fp8) {
                const size_t r1 = align_up(E, 256), r3 = align_up(3 * E, 256), r4 = align_up(4 * E, 256);
                b.wqkv = cv.take(r3 * E);
                b.wpan = cv.take(128 * E * 2);
                b.wo = cv.take(r1 * E); b.wfc = cv.take(r4 * E); b.wpr = cv.take(r1 * 4 * E);
                b.sqkv = cv.take(3 * E * 4); b.so = cv.take(E * 4); b.sfc = cv.take(4 * E * 4); b.spr = cv.take(E * 4);
            } else {
                const size_t es = c->es;
                b.wqkv = cv.take((size_t)c->NQpad * E * es);
                b.wo = cv.take(E * E * es); b.wfc = cv.take(4 * E * E * es); b.wpr = cv.take(4 * E * E * es);
            }
            b.wqkvT = b.woT = b.wfcT = b.wprT = b.wdT = b.wuT = 0;
            if (c->d.method != PEVIT_NONE) b.tsink = cv.take(64 * E * c->es);
        } else if (c->fp8) {
            // one byte per weight; rows padded to the largest tile (256) so that clamped tile rows stay readable
            const size_t r1 = align_up(E, 256), r3 = align_up(3 * E, 256), r4 = align_up(4 * E, 256);
            b.wqkv = cv.take(r3 * E);
            b.wpan = cv.take(128 * E * 2);
            b.wqkvT = cv.take(E * (size_t)c->NQ * 2);          // QKV backward keeps bf16: its K mixes frozen rows with the adapter panel
            b.wo = cv.take(r1 * E);       b.woT = cv.take(r1 * E);
            b.wfc = cv.take(r4 * E);      b.wfcT = cv.take(r1 * 4 * E);
            b.wpr = cv.take(r1 * 4 * E);  b.wprT = cv.take(r4 * E);
            b.sqkv = cv.take(3 * E * 4); b.so = cv.take(E * 4); b.sfc = cv.take(4 * E * 4); b.spr = cv.take(E * 4);
        } else {
            const size_t es = c->es;
            b.wqkv = cv.take((size_t)c->NQpad * E * es);
            b.wqkvT = cv.take(E * (size_t)c->NQ * es);
            b.wo = cv.take(E * E * es);   b.woT = cv.take(E * E * es);
            b.wfc = cv.take(4 * E * E * es); b.wfcT = cv.take(4 * E * E * es);
            b.wpr = cv.take(4 * E * E * es); b.wprT = cv.take(4 * E * E * es);
        }
        b.bqkv = cv.take(3 * E * 4); b.bo = cv.take(E * 4); b.bfc = cv.take(4 * E * 4); b.bpr = cv.take(E * 4);
        b.ln1w = cv.take(E * 4); b.ln1b = cv.take(E * 4); b.ln2w = cv.take(E * 4); b.ln2b = cv.take(E * 4);
        b.q32 = cv.take(E * 64 * 4); b.qT = cv.take(64 * E * c->es); b.q16 = cv.take(E * 64 * 2);
        b.q16s = site_slots(c) ? cv.take(site_slots(c) * q16_slot_bytes(c)) : 0;
        b.wds = b.wus = 0;
        if (c->infer_only) {
            b.wd = cv.take(64 * E * c->es); b.wu = cv.take(64 * E * c->es);
            // post-MLP slot context: the panels of every slot behind those of the single-adapter calls
            if (post_mlp(c) && c->slots) { b.wds = cv.take(c->slots * pm_slot_bytes(c)); b.wus = cv.take(c->slots * pm_slot_bytes(c)); }
            continue;
        }
        b.wd = cv.take(64 * E * c->es); b.wdT = cv.take(64 * E * c->es); b.wu = cv.take(64 * E * c->es); b.wuT = cv.take(64 * E * c->es);
    }
}

// the image-side and training entry points on a text context (its workspace holds the inference layout only, it has no stem, no
// head and no parameters), checked on the host before anything else
int refuse_text(const pevit_ctx* c, const char* who) {
    if (c && c->text) {
        pevit_set_error("%s: this is a text context (pevit_text_create); it runs pevit_encode_text only", who);
        return -1;
    }
    return 0;
}

// everything but the inference walk, its loaders and the queries on an inference-only context, checked on the host before anything else:
// nothing is launched, the flag words and the workspace stay as they are
int refuse_infer(const pevit_ctx* c, const char* who) {
    if (c && c->infer_only) {
        pevit_set_error("%s: this is an inference-only context (pevit_infer_create); it runs pevit_predict, pevit_encode_image and "
                        "pevit_zeroshot only", who);
        return -1;
    }
    return 0;
}

// a backward runs on the activations of the forward it asks for (kind, batch and, for the attention seam, layer) or is refused
int check_saved(const pevit_ctx* c, Saved want, int B, int layer, const char* who) {
    const SavedForward& f = c->saved;
    if (f.kind == want && f.batch == B && (want != Saved::attention || f.layer == layer)) return 0;
    static const char* const wanted[] = {"", "a blocks/transformer forward", "a visual_forward", "an attention_forward"};
    static const char* const name[] = {"none", "transformer_forward", "visual_forward", "attention_forward"};
    char want_l[32] = "", have_l[32] = "";
    if (want == Saved::attention) snprintf(want_l, sizeof(want_l), " of layer %d", layer);
    if (f.kind == Saved::attention) snprintf(have_l, sizeof(have_l), " of layer %d", f.layer);
    pevit_set_error("%s: the saved activations are not those of %s%s with batch %d (saved: batch %d, %s%s)", who, wanted[(int)want],
                    want_l, B, f.batch, name[(int)f.kind], have_l);
    return -1;
}

int check_ready(pevit_ctx* c, int B, const char* who) {
    if (!c || !c->arena || !c->ws) { pevit_set_error("%s: context not bound", who); return -1; }
    if (B <= 0 || B > c->max_batch) { pevit_set_error("%s: batch %d outside [1,%d]", who, B, c->max_batch); return -1; }
    if (c->d.method != PEVIT_NONE && (!c->params || (!c->grads && !c->infer_only))) { pevit_set_error("%s: parameters not set", who); return -1; }
    return 0;
}

}  // namespace pevit_host

using namespace pevit_host;

// ------------------------------------------------------------------------------------
// what pevit_ctx_create and pevit_infer_create share: the checks of the dims (errors under the caller's name `who`), the arena and the
// flat parameter layout.  No HIP call: sizes only.
static int create_image_ctx(const pevit_dims* dims, pevit_ctx** out, bool infer_only, const char* who, int slots = 0) {
    if (!dims || !out) { pevit_set_error("%s: null argument", who); return -1; }
    const pevit_dims d = *dims;
    if (slots < 0 || slots > PEVIT_MAX_SLOTS) { pevit_set_error("%s: %d slots outside [1,%d]", who, slots, PEVIT_MAX_SLOTS); return -1; }
    if (d.width <= 0 || d.width % 128 != 0 || d.width > 1024) {
        pevit_set_error("%s: width %d must be a multiple of 128 in (0,1024]", who, d.width); return -1;
    }
    if (d.layers <= 0 || d.patch <= 0 || d.resolution <= 0 || d.resolution % d.patch != 0) {
        pevit_set_error("%s: bad layers/patch/resolution %d/%d/%d", who, d.layers, d.patch, d.resolution); return -1;
    }
    if (d.method < 0 || d.method > PEVIT_NONE) { pevit_set_error("%s: unknown method %d", who, d.method); return -1; }
    if (d.method == PEVIT_LORA && (d.lora_rank < 1 || d.lora_rank > 32)) {
        pevit_set_error("%s: LoRA rank %d outside [1,32]", who, d.lora_rank); return -1;
    }
    if (d.weight_format != PEVIT_W_BF16 && d.weight_format != PEVIT_W_FP8_E4M3 && d.weight_format != PEVIT_W_F32_VERIFY &&
        d.weight_format != PEVIT_W_FP8_ACT) {
        pevit_set_error("%s: unknown weight_format %d", who, d.weight_format); return -1;
    }
    if ((d.weight_format == PEVIT_W_FP8_E4M3 || d.weight_format == PEVIT_W_FP8_ACT) && (d.method == PEVIT_ADAPTER || d.method == PEVIT_COMPACTER)) {
        pevit_set_error("%s: fp8 weights are built for the attention-site methods (KAdaptation, LoRA) and the frozen tower", who); return -1;
    }
    if (d.out_dim <= 0 || d.out_dim % 8 != 0 || d.num_classes <= 0) {
        pevit_set_error("%s: bad out_dim/num_classes %d/%d", who, d.out_dim, d.num_classes); return -1;
    }
    pevit_ctx* c = new (std::nothrow) pevit_ctx();
    if (!c) { pevit_set_error("%s: out of host memory", who); return -1; }
    c->d = d;
    c->infer_only = infer_only;
    c->E = d.width; c->L = d.layers; c->H = d.width / 64; c->P = d.patch; c->R = d.resolution;
    const int grid = d.resolution / d.patch;
    c->G2 = grid * grid; c->N = c->G2 + 1; c->D = d.out_dim; c->C = d.num_classes;
    c->Kpatch = (int)align_up((size_t)3 * d.patch * d.patch, 64);
    c->slots = slots;
    c->NQ = 3 * c->E + 64 * (site_slots(c) + 1); c->NQpad = (int)align_up((size_t)c->NQ, 128);
    c->ascale = d.method == PEVIT_LORA ? 128.0f / (float)d.lora_rank : 160.0f;
    c->fp8act = d.weight_format == PEVIT_W_FP8_ACT;
    c->fp8 = d.weight_format == PEVIT_W_FP8_E4M3 || c->fp8act;
    c->f32 = d.weight_format == PEVIT_W_F32_VERIFY;
    c->es = c->f32 ? 4 : 2;
    c->sk_slots = c->f32 ? 0 : pevit_gemm_sk_slots();
    if (c->N > 288) { pevit_set_error("%s: %d tokens per image exceeds 288", who, c->N); delete c; return -1; }

    // ---- weight arena -------------------------------------------------------------
    c->blk = new (std::nothrow) BlockArena[c->L];
    if (!c->blk) { pevit_set_error("%s: out of host memory", who); pevit_ctx_destroy(c); return -1; }
    Carver cv;
    const size_t E = c->E;
    carve_block_arena(c, cv);
    c->a_conv = cv.take(align_up(E, 128) * (size_t)c->Kpatch * c->es);
    c->a_cls = cv.take(E * 4);
    c->a_pos = cv.take((size_t)c->N * E * 4);
    c->a_lnpre_w = cv.take(E * 4); c->a_lnpre_b = cv.take(E * 4);
    c->a_lnpost_w = cv.take(E * 4); c->a_lnpost_b = cv.take(E * 4);
    c->a_proj = cv.take(align_up((size_t)c->D, 128) * E * c->es);      // [D][E]  (proj^T)
    c->a_projT = infer_only ? 0 : cv.take(E * (size_t)c->D * c->es);  // [E][D]: the backward's operand
    c->a_phm = cv.take(64 * 4);
    c->arena_bytes = cv.off;

    // ---- flat trainable parameters (reference named_parameters() order) -----------
    if (d.method == PEVIT_KADAPTATION) {
        c->p_layer0 = 4 * 32 * 32; c->p_layer_stride = 5 * E;
    } else if (d.method == PEVIT_LORA) {
        c->p_layer0 = 0; c->p_layer_stride = 4 * (size_t)d.lora_rank * E;
    } else if (d.method == PEVIT_ADAPTER) {
        // adapter_norm_before.{weight,bias}, adapter_down.1.{weight (64,E), bias}, adapter_up.{weight (E,64), bias}
        c->o_nw = 0; c->o_nb = E; c->o_dw = 2 * E; c->o_db = c->o_dw + 64 * E; c->o_uw = c->o_db + 64;
        c->o_ub = c->o_uw + 64 * E;
        c->p_layer0 = 0; c->p_layer_stride = c->o_ub + E;
    } else if (d.method == PEVIT_COMPACTER) {
        // adapter_norm_before.{weight,bias}, adapter_down.1.{W_left (4,E/4,1), W_right (4,1,16), b (64)},
        // adapter_up.{W_left (4,16,1), W_right (4,1,E/4), b (E)}
        c->o_nw = 0; c->o_nb = E; c->o_dWl = 2 * E; c->o_dWr = c->o_dWl + E; c->o_db = c->o_dWr + 64;
        c->o_uWl = c->o_db + 64; c->o_uWr = c->o_uWl + 64; c->o_ub = c->o_uWr + E;
        c->p_layer0 = 0; c->p_layer_stride = c->o_ub + E;
    } else {
        c->p_layer0 = 0; c->p_layer_stride = 0;
    }
    c->n_tower = c->p_layer0 + c->p_layer_stride * c->L;
    c->p_head_w = c->n_tower;
    c->p_head_b = c->p_head_w + (size_t)c->C * c->D;
    c->n_total = c->p_head_b + c->C;
    *out = c;
    return 0;
}

extern "C" int pevit_ctx_create(const pevit_dims* dims, pevit_ctx** out) { return create_image_ctx(dims, out, false, "ctx_create"); }

// An image context that can only infer (include/pevit_hip.h): the arena without the transposed copies, the third workspace layout
// (layout_workspace), parameters through pevit_set_infer_params.  dims->num_classes is the largest head it will serve.
extern "C" int pevit_infer_create(const pevit_dims* dims, pevit_ctx** out) { return create_image_ctx(dims, out, true, "infer_create"); }

// The same with `slots` resident adapters for pevit_predict_segments (include/pevit_segments.h): per layer 64 more rows of wqkv and
// one more Q panel per slot, 64 more f32 columns of t per slot and token.  What the segmented attention site was not built for is
// refused by name; with one slot such dims give the context of pevit_infer_create.
extern "C" int pevit_infer_create_slots(const pevit_dims* dims, int slots, pevit_ctx** out) {
    const char* who = "infer_create_slots";
    if (!dims || !out) { pevit_set_error("%s: null argument", who); return -1; }
    if (slots < 1 || slots > PEVIT_MAX_SLOTS) { pevit_set_error("%s: %d slots outside [1,%d]", who, slots, PEVIT_MAX_SLOTS); return -1; }
    const char* why = nullptr;
    if (dims->method == PEVIT_ADAPTER || dims->method == PEVIT_COMPACTER)
        why = "the post-MLP methods (Adapter, Compacter) are not served by segments: the 32-row blocks of their kernels straddle segments";
    else if (dims->method == PEVIT_NONE) why = "method none has no adapter to keep in a slot";
    else if (dims->weight_format == PEVIT_W_FP8_E4M3 || dims->weight_format == PEVIT_W_FP8_ACT)
        why = "the fp8 weight formats keep the adapter rows outside the QKV product; segments are built for bf16";
    else if (dims->weight_format == PEVIT_W_F32_VERIFY) why = "the f32 verification mode has no segmented kernels";
    if (why && slots > 1) { pevit_set_error("%s: %d slots: %s", who, slots, why); return -1; }
    return create_image_ctx(dims, out, true, who, why ? 0 : slots);
}

// Make `params` (the flat buffer of pevit_set_infer_params) resident in a slot: its bf16 panels are built here, once, by the kernel
// the walk launches per call for the selected adapter; the pointer is kept for the delta bias and the head.
extern "C" int pevit_load_adapter_slot(pevit_ctx* c, void* stream, int slot, const float* params, int num_classes) {
    if (!c || !params) { pevit_set_error("load_adapter_slot: null argument"); return -1; }
    if (!c->slots) { pevit_set_error("load_adapter_slot: this context has no adapter slots (pevit_infer_create_slots)"); return -1; }
    if (c->d.method == PEVIT_COMPACTER) {
        pevit_set_error("load_adapter_slot: a Compacter slot needs the adapter's frozen phm_rule: pevit_load_adapter_slot_rule takes it");
        return -1;
    }
    if (!c->arena) { pevit_set_error("load_adapter_slot: context not bound"); return -1; }
    if (slot < 0 || slot >= c->slots) { pevit_set_error("load_adapter_slot: slot %d outside [0,%d)", slot, c->slots); return -1; }
    if (num_classes < 1 || num_classes > c->d.num_classes) {
        pevit_set_error("load_adapter_slot: num_classes %d outside [1,%d] of the context", num_classes, c->d.num_classes); return -1;
    }
    c->slot_params[slot] = nullptr;
    CHECK(prep_adapters(c, (hipStream_t)stream, slot, params));
    c->slot_params[slot] = params; c->slot_classes[slot] = num_classes;
    return 0;
}

// Slot contexts for all four methods (include/pevit_segments_all.h).  The attention-site methods: pevit_infer_create_slots itself.
// The post-MLP methods: per layer and slot one down and one up panel in the arena (carve_block_arena: wds, wus); the workspace is
// that of pevit_infer_create.
extern "C" int pevit_infer_create_slots_all(const pevit_dims* dims, int slots, pevit_ctx** out) {
    const char* who = "infer_create_slots_all";
    if (!dims || !out) { pevit_set_error("%s: null argument", who); return -1; }
    if (dims->method == PEVIT_KADAPTATION || dims->method == PEVIT_LORA) return pevit_infer_create_slots(dims, slots, out);
    if (slots < 1 || slots > PEVIT_MAX_SLOTS) { pevit_set_error("%s: %d slots outside [1,%d]", who, slots, PEVIT_MAX_SLOTS); return -1; }
    const char* why = nullptr;
    if (dims->method == PEVIT_NONE) why = "method none has no adapter to keep in a slot";
    else if (dims->weight_format == PEVIT_W_FP8_E4M3 || dims->weight_format == PEVIT_W_FP8_ACT)
        why = "the fp8 weight formats are not served by segments; slots are built for bf16";
    else if (dims->weight_format == PEVIT_W_F32_VERIFY) why = "the f32 verification mode has no segmented kernels";
    if (why && slots > 1) { pevit_set_error("%s: %d slots: %s", who, slots, why); return -1; }
    return create_image_ctx(dims, out, true, who, (why || slots == 1) ? 0 : slots);
}

// pevit_load_adapter_slot with Compacter's frozen rule: read from the caller's buffer while the panels are built, never through
// the arena's a_phm (which belongs to the adapter the single-adapter calls selected).
extern "C" int pevit_load_adapter_slot_rule(pevit_ctx* c, void* stream, int slot, const float* params, int num_classes, const float* phm_rule) {
    const char* who = "load_adapter_slot_rule";
    if (!c || !params) { pevit_set_error("%s: null argument", who); return -1; }
    if (!c->slots) { pevit_set_error("%s: this context has no adapter slots (pevit_infer_create_slots_all)", who); return -1; }
    if (c->d.method == PEVIT_COMPACTER) {
        if (!phm_rule) { pevit_set_error("%s: a Compacter slot needs the adapter's frozen phm_rule", who); return -1; }
    } else if (phm_rule) {
        pevit_set_error("%s: only Compacter has a phm_rule; this context takes NULL (or pevit_load_adapter_slot)", who); return -1;
    }
    if (!c->arena) { pevit_set_error("%s: context not bound", who); return -1; }
    if (slot < 0 || slot >= c->slots) { pevit_set_error("%s: slot %d outside [0,%d)", who, slot, c->slots); return -1; }
    if (num_classes < 1 || num_classes > c->d.num_classes) {
        pevit_set_error("%s: num_classes %d outside [1,%d] of the context", who, num_classes, c->d.num_classes); return -1;
    }
    c->slot_params[slot] = nullptr;
    CHECK(prep_adapters(c, (hipStream_t)stream, slot, params, phm_rule));
    c->slot_params[slot] = params; c->slot_classes[slot] = num_classes;
    return 0;
}

// The CLIP text tower as a context: the block arena of pevit_ctx_create (method PEVIT_NONE) and, in place of the image stem, the f32
// token-embedding table, the positional embedding, ln_final and text_projection^T.  No HIP call: sizes only.
extern "C" int pevit_text_create(const pevit_text_dims* dims, pevit_ctx** out) {
    if (!dims || !out) { pevit_set_error("text_create: null argument"); return -1; }
    const pevit_text_dims d = *dims;
    if (d.width <= 0 || d.width % 128 != 0 || d.width > 1024) {
        pevit_set_error("text_create: width %d must be a multiple of 128 in (0,1024]", d.width); return -1;
    }
    if (d.layers <= 0) { pevit_set_error("text_create: bad layer count %d", d.layers); return -1; }
    if (d.context_length < 1 || d.context_length > 128) {
        pevit_set_error("text_create: context_length %d outside [1,128] (the causal attention kernel keeps K and V of a prompt in LDS)", d.context_length); return -1;
    }
    if (d.vocab_size < 1) { pevit_set_error("text_create: bad vocab_size %d", d.vocab_size); return -1; }
    if (d.out_dim <= 0 || d.out_dim % 8 != 0) { pevit_set_error("text_create: out_dim %d must be a positive multiple of 8", d.out_dim); return -1; }
    if (d.weight_format == PEVIT_W_FP8_E4M3 || d.weight_format == PEVIT_W_FP8_ACT) {
        pevit_set_error("text_create: the fp8 weight formats were built for the image towers; the text tower takes bf16 or f32-verify"); return -1;
    }
    if (d.weight_format != PEVIT_W_BF16 && d.weight_format != PEVIT_W_F32_VERIFY) {
        pevit_set_error("text_create: unknown weight_format %d", d.weight_format); return -1;
    }
    pevit_ctx* c = new (std::nothrow) pevit_ctx();
    if (!c) { pevit_set_error("text_create: out of host memory"); return -1; }
    c->d = pevit_dims{};
    c->d.width = d.width; c->d.layers = d.layers; c->d.out_dim = d.out_dim; c->d.method = PEVIT_NONE; c->d.num_classes = 1;
    c->d.weight_format = d.weight_format;
    c->text = true; c->causal = true; c->V = d.vocab_size;
    c->E = d.width; c->L = d.layers; c->H = d.width / 64; c->P = 0; c->R = 0;
    c->G2 = 0; c->N = d.context_length; c->D = d.out_dim; c->C = 1; c->Kpatch = 0;
    c->NQ = 3 * c->E + 64; c->NQpad = (int)align_up((size_t)c->NQ, 128);
    c->ascale = 0.f;
    c->f32 = d.weight_format == PEVIT_W_F32_VERIFY;
    c->es = c->f32 ? 4 : 2;
    c->sk_slots = c->f32 ? 0 : pevit_gemm_sk_slots();
    c->blk = new (std::nothrow) BlockArena[c->L];
    if (!c->blk) { pevit_set_error("text_create: out of host memory"); pevit_ctx_destroy(c); return -1; }
    Carver cv;
    const size_t E = c->E;
    carve_block_arena(c, cv);
    c->a_tok = cv.take((size_t)c->V * E * 4);                          // f32: the embedding is exact
    c->a_pos = cv.take((size_t)c->N * E * 4);
    c->a_lnpost_w = cv.take(E * 4); c->a_lnpost_b = cv.take(E * 4);    // ln_final
    c->a_proj = cv.take(align_up((size_t)c->D, 128) * E * c->es);      // [D][E]  (text_projection^T)
    c->a_conv = c->a_cls = c->a_lnpre_w = c->a_lnpre_b = c->a_projT = c->a_phm = 0;
    c->arena_bytes = cv.off;
    c->p_layer0 = 0; c->p_layer_stride = 0;
    c->n_tower = 0; c->p_head_w = 0; c->p_head_b = 0; c->n_total = 0;
    *out = c;
    return 0;
}

extern "C" void pevit_ctx_destroy(pevit_ctx* c) {
    if (!c) return;
    for (int i = 0; i < 2 * c->prof_cap; ++i) (void)hipEventDestroy(c->prof_ev[i]);
    delete[] c->prof_ev;
    delete[] c->prof_flops;
    delete[] c->prof_bytes;
    delete[] c->prof_ms;
    delete[] c->prof_shape;
    delete[] c->blk;
    delete c;
}

extern "C" size_t pevit_arena_bytes(const pevit_ctx* c) { return c ? c->arena_bytes : 0; }
extern "C" size_t pevit_workspace_bytes(const pevit_ctx* c, int batch) {
    if (!c || batch <= 0) return 0;
    return layout_workspace(c, batch, c->text).total;      // a text context is inference-only: batch counts prompts (pevit_infer_create: its own layout)
}
// what a caller must leave alone between two calls: layout_workspace carves it first, whatever the batch and the layout
extern "C" size_t pevit_workspace_state_bytes(const pevit_ctx* c) { return c ? WS_STATE_BYTES : 0; }
extern "C" size_t pevit_num_tower_params(const pevit_ctx* c) { return c ? c->n_tower : 0; }
extern "C" size_t pevit_num_params(const pevit_ctx* c) { return c ? c->n_total : 0; }
extern "C" size_t pevit_param_layer_offset(const pevit_ctx* c, int layer) {
    if (!c) return 0;
    if (layer >= c->L) return c->n_tower;
    return c->p_layer0 + c->p_layer_stride * (size_t)(layer < 0 ? 0 : layer);
}

extern "C" int pevit_param_grad_mask(const pevit_ctx* c, unsigned char* m, size_t n) {
    if (!c || !m || n != c->n_total) { pevit_set_error("param_grad_mask: size mismatch"); return -1; }
    memset(m, 1, n);
    if (c->d.method == PEVIT_KADAPTATION) {
        const size_t E = c->E;
        for (int l = 0; l < c->L; ++l) {
            const size_t base = c->p_layer0 + c->p_layer_stride * l;
            memset(m + base + 2 * E, 0, 2 * E);       // v_proj_adapter1_left/right
        }
    }
    return 0;
}

extern "C" int pevit_bind(pevit_ctx* c, void* arena, size_t arena_bytes, void* ws, size_t ws_bytes, int max_batch) {
    if (!c || !arena || !ws) { pevit_set_error("bind: null argument"); return -1; }
    if (arena_bytes < c->arena_bytes) { pevit_set_error("bind: arena too small (%zu < %zu)", arena_bytes, c->arena_bytes); return -1; }
    const size_t need = pevit_workspace_bytes(c, max_batch);
    if (ws_bytes < need) { pevit_set_error("bind: workspace too small (%zu < %zu)", ws_bytes, need); return -1; }
    if (((uintptr_t)arena | (uintptr_t)ws) & 255) { pevit_set_error("bind: buffers must be 256-byte aligned"); return -1; }
    c->arena = (char*)arena; c->ws = (char*)ws; c->max_batch = max_batch; c->ws_bytes_for_max = need;
    // whatever a forward saved lived in the workspace bound before: a backward through it is refused from here on
    c->saved = SavedForward{}; c->dfeatb_of = nullptr;
    // the stream-K flags must read 0 before the first launch (every launch leaves them 0 again)
    HIP_OK(hipMemset(c->ws, 0, WS_STATE_BYTES));
    return 0;
}

extern "C" int pevit_set_params(pevit_ctx* c, float* params, float* grads, float* mom, const unsigned char* mask) {
    CHECK(refuse_infer(c, "set_params"));
    if (!c || !params || !grads) { pevit_set_error("set_params: null argument"); return -1; }
    c->params = params; c->grads = grads; c->mom = mom; c->grad_mask = mask;
    return 0;
}

// The parameters of an inference-only context: params = [tower adapters in adapter_param_spec order | head W (C x D) | head b (C)],
// device f32, for 1 <= C <= dims.num_classes; the head offsets follow C.  Only read, by pointer: calling again swaps the adapter (the
// walk rebuilds the adapter panels from the flat buffer on every forward).
extern "C" int pevit_set_infer_params(pevit_ctx* c, const float* params, int num_classes) {
    if (!c || !params) { pevit_set_error("set_infer_params: null argument"); return -1; }
    if (!c->infer_only) { pevit_set_error("set_infer_params: not an inference-only context (pevit_infer_create); a training context takes pevit_set_params"); return -1; }
    if (num_classes < 1 || num_classes > c->d.num_classes) {
        pevit_set_error("set_infer_params: num_classes %d outside [1,%d] of the context", num_classes, c->d.num_classes); return -1;
    }
    c->params = const_cast<float*>(params);
    c->C = num_classes;
    c->p_head_w = c->n_tower;
    c->p_head_b = c->p_head_w + (size_t)c->C * c->D;
    c->n_total = c->p_head_b + c->C;
    return 0;
}

// ------------------------------------------------------------------------------------
extern "C" int pevit_load_block(pevit_ctx* c, void* stream, int l, const float* in_w, const float* in_b,
                                const float* out_w, const float* out_b, const float* ln1w, const float* ln1b,
                                const float* fc_w, const float* fc_b, const float* pr_w, const float* pr_b,
                                const float* ln2w, const float* ln2b) {
    if (!c || !c->arena) { pevit_set_error("load_block: context not bound"); return -1; }
    if (l < 0 || l >= c->L) { pevit_set_error("load_block: layer %d out of range", l); return -1; }
    hipStream_t s = (hipStream_t)stream;
    const BlockArena& b = c->blk[l];
    const size_t E = c->E;
    char* A = c->arena;
    // the 1/sqrt(head_dim) of model.py:786-787 is folded into the q rows (exact: a power of two)
    if (c->fp8) {
        typedef unsigned char u8;
        const int e = (int)E;
        HIP_OK(hipMemsetAsync(A + b.wqkv, 0, align_up(3 * E, 256) * E, s));
        HIP_OK(hipMemsetAsync(A + b.wpan, 0, 128 * E * 2, s));
        HIP_OK(hipMemsetAsync(A + b.wo, 0, align_up(E, 256) * E, s));
        HIP_OK(hipMemsetAsync(A + b.wfc, 0, align_up(4 * E, 256) * E, s));
        HIP_OK(hipMemsetAsync(A + b.wpr, 0, align_up(E, 256) * 4 * E, s));
        CHECK(pevit_launch_quant_rows_fp8(in_w, 3 * e, e, at<u8>(A, b.wqkv), e, at<float>(A, b.sqkv), e, 0.125f, s));
        CHECK(pevit_launch_quant_rows_fp8(out_w, e, e, at<u8>(A, b.wo), e, at<float>(A, b.so), 0, 1.0f, s));
        CHECK(pevit_launch_quant_rows_fp8(fc_w, 4 * e, e, at<u8>(A, b.wfc), e, at<float>(A, b.sfc), 0, 1.0f, s));
        CHECK(pevit_launch_quant_rows_fp8(pr_w, e, 4 * e, at<u8>(A, b.wpr), 4 * e, at<float>(A, b.spr), 0, 1.0f, s));
        // an inference-only context keeps no transposed copy, so its load needs no workspace scratch either
        if (!c->infer_only) {
            HIP_OK(hipMemsetAsync(A + b.woT, 0, align_up(E, 256) * E, s));
            HIP_OK(hipMemsetAsync(A + b.wfcT, 0, align_up(E, 256) * 4 * E, s));
            HIP_OK(hipMemsetAsync(A + b.wprT, 0, align_up(4 * E, 256) * E, s));
            CHECK(pevit_launch_quant_transpose_fp8(out_w, e, e, at<float>(A, b.so), at<u8>(A, b.woT), e, 0, 1.0f, s));
            CHECK(pevit_launch_quant_transpose_fp8(fc_w, 4 * e, e, at<float>(A, b.sfc), at<u8>(A, b.wfcT), 4 * e, 0, 1.0f, s));
            CHECK(pevit_launch_quant_transpose_fp8(pr_w, e, 4 * e, at<float>(A, b.spr), at<u8>(A, b.wprT), e, 0, 1.0f, s));
            // QKV backward (bf16): the transposed copy holds the DE-QUANTISED weights, exactly representable in bf16
            HIP_OK(hipMemsetAsync(A + b.wqkvT, 0, E * (size_t)c->NQ * 2, s));
            const size_t skip = align_up(WS_STATE_BYTES, 256);    // the stream-K flags stay zero
            // 3E*E floats of the bound workspace serve as packing scratch: whatever activations a previous forward saved there
            // are overwritten, so a backward through them is refused from here on, and the load must be
            // issued on the stream the engine trains on (include/pevit_hip.h: one stream per context)
            float* tmp = at<float>(c->ws, skip);
            c->saved = SavedForward{};
            if (skip + (size_t)3 * E * E * 4 > c->ws_bytes_for_max) { pevit_set_error("load_block: workspace too small for the fp8 packing scratch"); return -1; }
            CHECK(pevit_launch_dequant_rows_fp8(at<u8>(A, b.wqkv), e, at<float>(A, b.sqkv), 3 * e, e, tmp, s));
            CHECK(pevit_launch_transpose_bf16(tmp, 3 * e, e, at<bf16>(A, b.wqkvT), c->NQ, 0, 1.0f, s));
        }
    } else {
        const int f = c->f32;
        HIP_OK(hipMemsetAsync(A + b.wqkv, 0, (size_t)c->NQpad * E * c->es, s));
        CHECK(pevit_launch_cast_bf16(in_w, at<bf16>(A, b.wqkv), E * E, 0.125f, s, f));
        CHECK(pevit_launch_cast_bf16(in_w + E * E, eadv(c, at<bf16>(A, b.wqkv), E * E), 2 * E * E, 1.0f, s, f));
        CHECK(pevit_launch_cast_bf16(out_w, at<bf16>(A, b.wo), E * E, 1.0f, s, f));
        CHECK(pevit_launch_cast_bf16(fc_w, at<bf16>(A, b.wfc), 4 * E * E, 1.0f, s, f));
        CHECK(pevit_launch_cast_bf16(pr_w, at<bf16>(A, b.wpr), 4 * E * E, 1.0f, s, f));
        if (!c->infer_only) {           // the transposed copies: operands of the dX products
            HIP_OK(hipMemsetAsync(A + b.wqkvT, 0, E * (size_t)c->NQ * c->es, s));
            CHECK(pevit_launch_transpose_bf16(in_w, 3 * (int)E, (int)E, at<bf16>(A, b.wqkvT), c->NQ, (int)E, 0.125f, s, f));
            CHECK(pevit_launch_transpose_bf16(out_w, (int)E, (int)E, at<bf16>(A, b.woT), (int)E, 0, 1.0f, s, f));
            CHECK(pevit_launch_transpose_bf16(fc_w, 4 * (int)E, (int)E, at<bf16>(A, b.wfcT), 4 * (int)E, 0, 1.0f, s, f));
            CHECK(pevit_launch_transpose_bf16(pr_w, (int)E, 4 * (int)E, at<bf16>(A, b.wprT), (int)E, 0, 1.0f, s, f));
        }
    }
    // biases and LN affines stay f32; the q third of in_proj_bias carries the same 1/8
    HIP_OK(hipMemcpyAsync(A + b.bqkv, in_b, 3 * E * 4, hipMemcpyDeviceToDevice, s));
    CHECK(pevit_launch_scale_f32(at<float>(A, b.bqkv), E, 0.125f, s));
    HIP_OK(hipMemcpyAsync(A + b.bo, out_b, E * 4, hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemcpyAsync(A + b.bfc, fc_b, 4 * E * 4, hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemcpyAsync(A + b.bpr, pr_b, E * 4, hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemcpyAsync(A + b.ln1w, ln1w, E * 4, hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemcpyAsync(A + b.ln1b, ln1b, E * 4, hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemcpyAsync(A + b.ln2w, ln2w, E * 4, hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemcpyAsync(A + b.ln2b, ln2b, E * 4, hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemsetAsync(A + b.q32, 0, E * 64 * 4, s));
    HIP_OK(hipMemsetAsync(A + b.qT, 0, 64 * E * c->es, s));
    HIP_OK(hipMemsetAsync(A + b.q16, 0, E * 64 * 2, s));
    for (int i = 0; i < c->slots; ++i) c->slot_params[i] = nullptr;       // (the rows of every slot went with the wqkv memset)
    return 0;
}

extern "C" int pevit_set_optim_state(pevit_ctx* c, float* exp_avg_sq, const unsigned char* group_of) {
    CHECK(refuse_infer(c, "set_optim_state"));
    if (!c || !group_of) { pevit_set_error("set_optim_state: null argument"); return -1; }
    c->exp_avg_sq = exp_avg_sq; c->group_of = group_of;
    return 0;
}

// a device word owned by the caller (e.g. pevit_ar_error_word) that, while non-zero, makes pevit_sgd_step withhold the update --
// the same treatment a stream-K hand-off error gets.  nullptr detaches it.  The word must outlive the context's use of it.
extern "C" int pevit_set_external_poison(pevit_ctx* c, const unsigned* device_word) {
    CHECK(refuse_infer(c, "set_external_poison"));
    if (!c) { pevit_set_error("set_external_poison: null context"); return -1; }
    c->ext_poison = device_word;
    return 0;
}

// Round 5, data parallelism: an event the FUSED step (pevit_train_forward_backward[_u8]) waits for on its stream AFTER the stem
// (patch gather, patch embedding, class / position rows, ln_pre -- nothing of which reads a trainable parameter or touches the
// gradient buffer) and BEFORE the first use of the adapters and the clearing of the gradients.  The caller records it behind the
// previous step's gradient exchange + optimizer update, which it may then run on another stream: the exchange's latency and its
// cross-stream hand-overs run under ~70 us of the next step's stem instead of between two steps.  nullptr detaches it.
extern "C" int pevit_set_step_gate(pevit_ctx* c, void* event) {
    CHECK(refuse_infer(c, "set_step_gate"));
    if (!c) { pevit_set_error("set_step_gate: null context"); return -1; }
    c->step_gate = (hipEvent_t)event;
    return 0;
}

// ------------------------------------------------------------------------------------
extern "C" int pevit_load_stem(pevit_ctx* c, void* stream, const float* conv_w, const float* cls, const float* pos,
                               const float* lnpre_w, const float* lnpre_b, const float* lnpost_w, const float* lnpost_b,
                               const float* proj) {
    CHECK(refuse_text(c, "load_stem"));
    if (!c || !c->arena) { pevit_set_error("load_stem: context not bound"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    char* A = c->arena;
    const size_t E = c->E;
    CHECK(pevit_launch_conv_weight(conv_w, at<bf16>(A, c->a_conv), c->E, 3 * c->P * c->P, c->Kpatch, s, c->f32));
    HIP_OK(hipMemcpyAsync(A + c->a_cls, cls, E * 4, hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemcpyAsync(A + c->a_pos, pos, (size_t)c->N * E * 4, hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemcpyAsync(A + c->a_lnpre_w, lnpre_w, E * 4, hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemcpyAsync(A + c->a_lnpre_b, lnpre_b, E * 4, hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemcpyAsync(A + c->a_lnpost_w, lnpost_w, E * 4, hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemcpyAsync(A + c->a_lnpost_b, lnpost_b, E * 4, hipMemcpyDeviceToDevice, s));
    // proj is (E, D): feat = x @ proj  ->  B operand [D][E] = proj^T ; backward uses proj itself [E][D]
    CHECK(pevit_launch_transpose_bf16(proj, c->E, c->D, at<bf16>(A, c->a_proj), c->E, 0, 1.0f, s, c->f32));
    if (!c->infer_only) CHECK(pevit_launch_cast_bf16(proj, at<bf16>(A, c->a_projT), E * (size_t)c->D, 1.0f, s, c->f32));
    return 0;
}

extern "C" int pevit_load_phm_rule(pevit_ctx* c, void* stream, const float* phm_rule) {
    CHECK(refuse_text(c, "load_phm_rule"));
    if (!c || !c->arena) { pevit_set_error("load_phm_rule: context not bound"); return -1; }
    HIP_OK(hipMemcpyAsync(c->arena + c->a_phm, phm_rule, 64 * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// Preprocessing constants of the uint8 entry points: x = (u8 / 255 - mean[c]) / std[c], the dataset transforms of the reference
// (ToTensor + Normalize(INPUT.MEAN, INPUT.STD), feature.py:537-542; resources/model/vitb32_CLIP.yaml:4-6)
extern "C" int pevit_set_input_norm(pevit_ctx* c, const float* mean3, const float* std3) {
    CHECK(refuse_text(c, "set_input_norm"));
    if (!c || !mean3 || !std3) { pevit_set_error("set_input_norm: null argument"); return -1; }
    for (int i = 0; i < 3; ++i) {
        if (!(std3[i] > 0.f)) { pevit_set_error("set_input_norm: std[%d] = %g must be positive", i, (double)std3[i]); return -1; }
        c->img_mean[i] = mean3[i]; c->img_std[i] = std3[i];
    }
    c->img_norm_set = true;
    return 0;
}

// ---- the CLIP text tower (pevit_text_create) ---------------------------------------------------------------------------------
extern "C" int pevit_load_text_stem(pevit_ctx* c, void* stream, const float* token_embedding, const float* positional_embedding,
                                    const float* ln_final_weight, const float* ln_final_bias, const float* text_projection) {
    if (!c || !c->text) { pevit_set_error("load_text_stem: not a text context (pevit_text_create)"); return -1; }
    if (!c->arena) { pevit_set_error("load_text_stem: context not bound"); return -1; }
    if (!token_embedding || !positional_embedding || !ln_final_weight || !ln_final_bias || !text_projection) {
        pevit_set_error("load_text_stem: null argument"); return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    char* A = c->arena;
    const size_t E = c->E;
    HIP_OK(hipMemcpyAsync(A + c->a_tok, token_embedding, (size_t)c->V * E * 4, hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemcpyAsync(A + c->a_pos, positional_embedding, (size_t)c->N * E * 4, hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemcpyAsync(A + c->a_lnpost_w, ln_final_weight, E * 4, hipMemcpyDeviceToDevice, s));
    HIP_OK(hipMemcpyAsync(A + c->a_lnpost_b, ln_final_bias, E * 4, hipMemcpyDeviceToDevice, s));
    // text_projection is (E, D): features = x @ text_projection  ->  B operand [D][E] = its transpose, like visual.proj
    HIP_OK(hipMemsetAsync(A + c->a_proj, 0, align_up((size_t)c->D, 128) * E * c->es, s));
    CHECK(pevit_launch_transpose_bf16(text_projection, c->E, c->D, at<bf16>(A, c->a_proj), c->E, 0, 1.0f, s, c->f32));
    return 0;
}

extern "C" int pevit_tune(pevit_ctx* c, const char* key, int value) {
    static const struct { const char* key; int GemmTune::*field; } gemm_keys[] = {
        {"gemm_config", &GemmTune::config}, {"gemm_persistent", &GemmTune::persistent}, {"gemm_ablate", &GemmTune::ablate},
        {"gemm_kswitch", &GemmTune::kswitch}, {"gemm_big", &GemmTune::big}, {"gemm_cfg_longk", &GemmTune::cfg_longk},
        {"gemm_cfg_shortk", &GemmTune::cfg_shortk}, {"gemm_big_bias", &GemmTune::big_bias}, {"gemm_streamk", &GemmTune::streamk},
        {"gemm_sk_share", &GemmTune::sk_share}, {"gemm_sk_band", &GemmTune::sk_band}, {"gemm_ksplit", &GemmTune::ksplit},
        {"gemm_ksplit_small", &GemmTune::ksplit_small}, {"gemm_ksplit_stagger", &GemmTune::ksplit_stagger},
        {"gemm_ksplit_mink", &GemmTune::ksplit_mink}, {"gemm_kphase_nl", &GemmTune::kphase_nl}, {"gemm_kz2", &GemmTune::kz2},
        {"gemm_skinny", &GemmTune::skinny}, {"gemm_skinny_maxm", &GemmTune::skinny_maxm}, {"gemm_skinny_mink", &GemmTune::skinny_mink},
        {"gemm_skinny_slices", &GemmTune::skinny_slices}, {"gemm_band", &GemmTune::band}, {"gemm_stagger", &GemmTune::stagger},
    };
    // these need a context
    static const struct { const char* key; int pevit_ctx::*field; } ctx_keys[] = {
        {"dx_stored", &pevit_ctx::dx_stored}, {"gstream_bf16", &pevit_ctx::gstream16}, {"profile_all", &pevit_ctx::prof_all}, {"fused_attn_delta", &pevit_ctx::fused_attn_delta},
        {"fp8_tail", &pevit_ctx::fp8_tail}, {"adapter_fused", &pevit_ctx::adapter_fused}, {"adapter_tn_fold", &pevit_ctx::adapter_tn_fold},
        {"lowrank_combo", &pevit_ctx::lowrank_combo}, {"lowrank_xcd", &pevit_ctx::lowrank_xcd},
    };
    GemmTune& t = c ? c->tune : g_default_tune;
    for (const auto& k : gemm_keys)
        if (key && !strcmp(key, k.key)) { t.*k.field = value; return 0; }
    for (const auto& k : ctx_keys)
        if (key && c && !strcmp(key, k.key)) { c->*k.field = value; return 0; }
    pevit_set_error("tune: unknown key %s", key ? key : "(null)");
    return -1;
}
