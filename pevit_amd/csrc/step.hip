// The extern "C" calls that run a forward or a backward: the blocks, transformer and attention seams, the visual tower, predict,
// the text tower, the head, the fused training step and the optimizer updates.
#include <math.h>

#include "host_ctx.h"

using namespace pevit_host;

// uint8 images need a context that knows their preprocessing constants
static int check_u8_input(const pevit_ctx* c, const char* who) {
    CHECK(refuse_text(c, who));
    if (c && !c->img_norm_set) { pevit_set_error("%s: call pevit_set_input_norm first", who); return -1; }
    return 0;
}
// blocks [l_lo, l_hi) of the tower; `what`: "block" or "layer", as the caller's messages have always named them
static int check_range(const pevit_ctx* c, int l_lo, int l_hi, const char* who, const char* what) {
    if (l_lo < 0 || l_hi > c->L || l_lo >= l_hi) { pevit_set_error("%s: bad %s range [%d, %d)", who, what, l_lo, l_hi); return -1; }
    return 0;
}
static int check_layer(const pevit_ctx* c, int layer, const char* who) {
    if (layer < 0 || layer >= c->L) { pevit_set_error("%s: layer %d outside [0, %d)", who, layer, c->L); return -1; }
    return 0;
}

// Blocks [l_lo, l_hi) of the tower on (N,B,E) activations: ResidualAttentionBlock.forward (model.py:972-975) for one block,
// Transformer.forward (model.py:1013) for all of them.  Every block keeps its own saved activations, so the blocks can be
// walked one call at a time (reference-side code that iterates visual.transformer.resblocks) and differentiated in reverse.
extern "C" int pevit_blocks_forward(pevit_ctx* c, void* stream, const float* x_nbe, float* y_nbe, int B, int save_for_backward,
                                    int l_lo, int l_hi) {
    CHECK(refuse_text(c, "blocks_forward"));
    CHECK(refuse_infer(c, "blocks_forward"));
    CHECK(check_ready(c, B, "blocks_forward"));
    CHECK(check_range(c, l_lo, l_hi, "blocks_forward", "block"));
    hipStream_t s = (hipStream_t)stream;
    c->lay = layout_workspace(c, B);
    const StepPlan pl = plan_step(c, B);
    CHECK(pevit_launch_permute_rows(x_nbe, at<float>(c->ws, c->lay.sav[l_lo].x_in), c->N, B, c->E, 1, s));
    CHECK(blocks_forward(c, s, B, pl, false, l_lo, l_hi));
    const size_t out = l_hi < c->L ? c->lay.sav[l_hi].x_in : c->lay.w_xfinal;
    CHECK(pevit_launch_permute_rows(at<float>(c->ws, out), y_nbe, c->N, B, c->E, 0, s));
    c->saved = SavedForward{Saved::blocks, save_for_backward ? B : 0, -1, pl};
    return 0;
}

extern "C" int pevit_transformer_forward(pevit_ctx* c, void* stream, const float* x_nbe, float* y_nbe, int B,
                                         int save_for_backward) {
    return pevit_blocks_forward(c, stream, x_nbe, y_nbe, B, save_for_backward, 0, c ? c->L : 0);
}

// dy (gradient of the output of block l_hi-1) -> dx (gradient of the input of block l_lo, may be NULL); the adapter gradients of
// exactly these blocks are accumulated into the flat gradient buffer
extern "C" int pevit_blocks_backward(pevit_ctx* c, void* stream, const float* dy_nbe, float* dx_nbe, int B, int l_lo, int l_hi) {
    CHECK(refuse_text(c, "blocks_backward"));
    CHECK(refuse_infer(c, "blocks_backward"));
    CHECK(check_ready(c, B, "blocks_backward"));
    CHECK(check_range(c, l_lo, l_hi, "blocks_backward", "block"));
    CHECK(check_saved(c, Saved::blocks, B, -1, "blocks_backward"));
    hipStream_t s = (hipStream_t)stream;
    const size_t n = (size_t)B * c->N * c->E;
    CHECK(pevit_launch_permute_rows(dy_nbe, at<float>(c->ws, c->lay.w_dxa), c->N, B, c->E, 1, s));
    if (c->fp8)
        CHECK(pevit_launch_cast_bf16_cols(at<float>(c->ws, c->lay.w_dxa), at<bf16>(c->ws, c->lay.w_dyb), (size_t)B * c->N, c->E,
                                          at<float>(c->arena, c->blk[l_hi - 1].spr), s));
    else
        CHECK(pevit_launch_cast_bf16(at<float>(c->ws, c->lay.w_dxa), at<bf16>(c->ws, c->lay.w_dyb), n, 1.0f, s, c->f32));
    CHECK(blocks_backward(c, s, B, c->saved.plan, dx_nbe != nullptr, false, l_hi, l_lo));
    if (dx_nbe) CHECK(pevit_launch_permute_rows(at<float>(c->ws, c->lay.w_dxa), dx_nbe, c->N, B, c->E, 0, s));
    return 0;
}

// MultiheadAttention.forward(x, x, x, need_weights, attn_mask=None, average_attn_weights) of block `layer` (model.py:837-944 ->
// 612-834) on (N,B,E) activations: the attention half of the block walk (the same QKV / delta / attention launches) between a cast of
// the caller's input into the layer's xn1 slot and out_proj + bias into f32, without the residual.  The layer's saved slots hold
// the activations; the softmax probabilities are recomputed from q, k and lse (attn_probs.hip) when asked for.
extern "C" int pevit_attention_forward(pevit_ctx* c, void* stream, int layer, const float* x_nbe, float* y_nbe, int B,
                                       int save_for_backward, float* weights, int average_weights) {
    CHECK(refuse_text(c, "attention_forward"));
    CHECK(refuse_infer(c, "attention_forward"));
    CHECK(check_ready(c, B, "attention_forward"));
    CHECK(check_layer(c, layer, "attention_forward"));
    if (c->fp8act) {
        pevit_set_error("attention_forward: weight format fp8-act is not supported by the attention seam (its e4m3 activation codes "
                        "come out of the LayerNorm kernel, which the seam does not run): use bf16, fp8 or f32-verify");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    c->lay = layout_workspace(c, B);
    const StepPlan pl = plan_step(c, B);
    const int E = c->E, N = c->N, T = B * N;
    char* W = c->ws; char* A = c->arena;
    const BlockArena& b = c->blk[layer];
    const LayerSaved& v = c->lay.sav[layer];
    float* xin = at<float>(W, c->lay.w_dxn);          // [T][E] f32 scratch (free in a forward pass)
    float* yout = at<float>(W, c->lay.w_dxa);
    CHECK(pevit_launch_permute_rows(x_nbe, xin, N, B, E, 1, s));
    CHECK(pevit_launch_cast_bf16(xin, at<bf16>(W, v.xn1), (size_t)T * E, 1.0f, s, c->f32));
    if (pl.site) CHECK(prep_adapters(c, s));
    CHECK(attn_core_fwd(c, s, B, pl, layer, nullptr, nullptr));
    if (weights) {
        AttnArgs a = attn_args(c, B, layer);
        a.probs = weights; a.average = average_weights ? 1 : 0;
        CHECK(c->f32 ? pevit_launch_attn_probs_f32(a, s) : pevit_launch_attn_probs(a, s));
    }
    {
        GemmParams p = gpw(c, at<bf16>(W, v.attn_out), E, b.wo, E, E, T, E, E, b.so);
        p.bias = at<float>(A, b.bo); p.outf = yout; p.ldo = E;
        CHECK(gemm(c, EPI_BIAS_F32, p, s));
    }
    CHECK(pevit_launch_permute_rows(yout, y_nbe, N, B, E, 0, s));
    c->saved = SavedForward{Saved::attention, save_for_backward ? B : 0, layer, pl};
    return 0;
}

// dy (gradient of out_proj's output) -> dx (gradient of the attention input, may be NULL); the adapter gradients of `layer` are
// accumulated into the flat gradient buffer exactly as pevit_blocks_backward over [layer, layer + 1) does (incl. its share of the
// shared phm_rule factors).  Adapter / Compacter / the frozen tower: stock attention with frozen weights, dx only.
extern "C" int pevit_attention_backward(pevit_ctx* c, void* stream, int layer, const float* dy_nbe, float* dx_nbe, int B) {
    CHECK(refuse_text(c, "attention_backward"));
    CHECK(refuse_infer(c, "attention_backward"));
    CHECK(check_ready(c, B, "attention_backward"));
    CHECK(check_layer(c, layer, "attention_backward"));
    CHECK(check_saved(c, Saved::attention, B, layer, "attention_backward"));
    const StepPlan& pl = c->saved.plan;
    hipStream_t s = (hipStream_t)stream;
    const int E = c->E, N = c->N, T = B * N;
    char* W = c->ws;
    float* dy = at<float>(W, c->lay.w_dxa);
    CHECK(pevit_launch_permute_rows(dy_nbe, dy, N, B, E, 1, s));
    // fp8: out_proj's channel scales ride on the A operand of its dX product (as LayerNorm backward leaves them in the block walk)
    if (c->fp8)
        CHECK(pevit_launch_cast_bf16_cols(dy, at<bf16>(W, c->lay.w_dyb), (size_t)T, E, at<float>(c->arena, c->blk[layer].so), s));
    else
        CHECK(pevit_launch_cast_bf16(dy, at<bf16>(W, c->lay.w_dyb), (size_t)T * E, 1.0f, s, c->f32));
    AttnGradWalk walk;
    CHECK(attn_core_bwd(c, s, B, pl, layer, false, walk));
    float* dx = at<float>(W, c->lay.w_dxb);
    if (dx_nbe) CHECK(attn_qkv_dx(c, s, B, pl, layer, dx));
    CHECK(attn_walk_end(c, s, B, walk));
    if (pl.site) CHECK(reduce_adapter_grads(c, s, B, pl, layer, layer + 1));
    if (dx_nbe) CHECK(pevit_launch_permute_rows(dx, dx_nbe, N, B, E, 0, s));
    return 0;
}

extern "C" int pevit_transformer_backward(pevit_ctx* c, void* stream, const float* dy_nbe, float* dx_nbe, int B) {
    return pevit_blocks_backward(c, stream, dy_nbe, dx_nbe, B, 0, c ? c->L : 0);
}

extern "C" int pevit_zero_grads(pevit_ctx* c, void* stream) {
    CHECK(refuse_infer(c, "zero_grads"));
    if (!c || !c->grads) { pevit_set_error("zero_grads: parameters not set"); return -1; }
    CHECK(pevit_launch_zero(c->grads, c->n_total * sizeof(float), (hipStream_t)stream));
    return 0;
}

extern "C" int pevit_sgd_step(pevit_ctx* c, void* stream, float lr, float momentum, float wd, float grad_scale,
                              int flags) {
    CHECK(refuse_infer(c, "sgd_step"));
    if (!c || !c->params || !c->grads || !c->mom) { pevit_set_error("sgd_step: parameters/momentum not set"); return -1; }
    // the error word of the workspace bound NOW (a re-bind moves it; without stream-K slots -- f32 verification mode -- there is
    // no hand-off that could fail and nothing to guard)
    unsigned* poison = (c->ws && c->sk_slots) ? at<unsigned>(c->ws, c->lay.w_skflag) + c->sk_slots : nullptr;
    unsigned* skipped = poison ? at<unsigned>(c->ws, c->lay.w_skflag) + PEVIT_SK_MAX_SLOTS + 1 : nullptr;
    float* loss_slot = c->last_loss; c->last_loss = nullptr;
    SgdArgs a;
    a.p = c->params; a.g = c->grads; a.mom = c->mom; a.has_grad = c->grad_mask; a.n = c->n_total;
    a.lr = lr; a.momentum = momentum; a.wd = wd; a.first_step = flags; a.grad_scale = grad_scale;
    a.poison = poison; a.skipped = skipped; a.poison2 = c->ext_poison;
    if (poison || c->ext_poison) a.loss_slot = loss_slot;
    return pevit_launch_sgd(a, (hipStream_t)stream);
}

// clip_grad_norm_ over the gradient buffer, between the backward (and the exchange) and the update: two launches of clip.hip.
// Neither error word gates it -- they withhold the update behind it, and a clipped buffer nobody applies harms nothing.
extern "C" int pevit_clip_grad_norm(pevit_ctx* c, void* stream, float max_norm, float grad_scale, float* scratch) {
    if (!c) { pevit_set_error("clip_grad_norm: null context"); return -1; }
    CHECK(refuse_text(c, "clip_grad_norm"));
    CHECK(refuse_infer(c, "clip_grad_norm"));
    CHECK(pevit_clip_check(max_norm, grad_scale, "clip_grad_norm"));
    if (!scratch) { pevit_set_error("clip_grad_norm: null scratch buffer (pevit_clip_scratch_floats)"); return -1; }
    if (!c->params || !c->grads || !c->n_total) { pevit_set_error("clip_grad_norm: parameters not set (pevit_set_params)"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    ClipArgs a;
    a.g = c->grads; a.mask = c->grad_mask; a.n = c->n_total; a.max_norm = max_norm; a.grad_scale = grad_scale; a.scratch = scratch;
    const double bytes = 4.0 * (double)a.n + (a.mask ? (double)a.n : 0.0);
    PROF(c, s, PEVIT_PROF_GRAD_SUMSQ, 1, bytes, pevit_launch_grad_sumsq(a, s));
    PROF(c, s, PEVIT_PROF_GRAD_SCALE, 1, bytes + 4.0 * (double)a.n, pevit_launch_grad_scale(a, s));
    return 0;
}

static_assert((int)PEVIT_OPTIM_SGD == (int)OPTIM_SGD && (int)PEVIT_OPTIM_ADAM == (int)OPTIM_ADAM &&
              (int)PEVIT_OPTIM_ADAMW == (int)OPTIM_ADAMW && PEVIT_OPTIM_MAX_GROUPS == OPTIM_MAX_GROUPS, "optimizer kinds: header vs kernels.h");

// Adam / AdamW / per-group SGD: one launch of optim_kernel (optim.hip).  Everything that is a function of the hyper-parameters
// and the step alone is computed here in double and rounded to f32 once.
extern "C" int pevit_optim_step(pevit_ctx* c, void* stream, int kind, const pevit_optim_group* groups, int n_groups, int step,
                                float grad_scale, int flags) {
    CHECK(refuse_infer(c, "optim_step"));
    if (!c || !c->params || !c->grads || !c->mom) { pevit_set_error("optim_step: parameters/momentum not set"); return -1; }
    if (kind != PEVIT_OPTIM_SGD && kind != PEVIT_OPTIM_ADAM && kind != PEVIT_OPTIM_ADAMW) {
        pevit_set_error("optim_step: unknown optimizer kind %d", kind); return -1;
    }
    const bool adam = kind != PEVIT_OPTIM_SGD;
    if (!groups || n_groups < 1 || n_groups > PEVIT_OPTIM_MAX_GROUPS) {
        pevit_set_error("optim_step: %d parameter groups (1 to %d are supported)", n_groups, PEVIT_OPTIM_MAX_GROUPS); return -1;
    }
    if (adam && step < 1) { pevit_set_error("optim_step: step %d (the Adam kinds count updates from 1)", step); return -1; }
    if (!c->group_of || (adam && !c->exp_avg_sq)) { pevit_set_error("optim_step: optimizer state not set (pevit_set_optim_state)"); return -1; }
    unsigned* poison = (c->ws && c->sk_slots) ? at<unsigned>(c->ws, c->lay.w_skflag) + c->sk_slots : nullptr;
    unsigned* skipped = poison ? at<unsigned>(c->ws, c->lay.w_skflag) + PEVIT_SK_MAX_SLOTS + 1 : nullptr;
    float* loss_slot = c->last_loss; c->last_loss = nullptr;
    OptimArgs a;
    a.p = c->params; a.g = c->grads; a.exp_avg = c->mom; a.exp_avg_sq = c->exp_avg_sq; a.group_of = c->group_of; a.n = c->n_total;
    a.kind = kind; a.n_groups = n_groups; a.first_step = flags & 1; a.grad_scale = grad_scale;
    a.poison = poison; a.skipped = skipped; a.poison2 = c->ext_poison;
    if (poison || c->ext_poison) a.loss_slot = loss_slot;
    for (int k = 0; k < n_groups; ++k) {
        const pevit_optim_group& h = groups[k];
        OptimGroup& o = a.groups[k];
        o.lr = (float)h.lr; o.wd = (float)h.weight_decay; o.momentum = (float)h.momentum; o.nesterov = h.nesterov != 0;
        if (!adam) continue;
        o.w1 = (float)(1.0 - h.beta1); o.beta2 = (float)h.beta2; o.w2 = (float)(1.0 - h.beta2); o.eps = (float)h.eps;
        o.step_size = (float)(h.lr / (1.0 - pow(h.beta1, (double)step)));
        o.sqrt_bc2 = (float)sqrt(1.0 - pow(h.beta2, (double)step));
        o.decay = (float)(1.0 - h.lr * h.weight_decay);
    }
    return pevit_launch_optim(a, (hipStream_t)stream);
}

// images (B,3,R,R) f32 -> feat (B,D) f32                               model.py:1034-1051
// infer (pevit_predict): the inference layout and kernel forms; what a previous forward saved is overwritten, so no backward may follow
// gate (the fused step, where pevit_set_step_gate gave it an event): wait for the step gate behind the stem and clear the gradients there
// segments (pevit_predict_segments, which has made its own checks: no adapter need be selected there): c->segs holds the call's segments
static int visual_forward_impl(pevit_ctx* c, void* stream, const void* images_any, int u8, float* feat, int B, int save_for_backward,
                               bool infer, bool gate, bool segments = false) {
    const float* images = (const float*)images_any;
    CHECK(refuse_text(c, infer ? "predict" : "visual_forward"));
    if (!segments) CHECK(check_ready(c, B, infer ? "predict" : "visual_forward"));
    hipStream_t s = (hipStream_t)stream;
    if (infer) c->saved = SavedForward{};
    c->lay = layout_workspace(c, B, infer);
    if (infer && c->lay.total > c->ws_bytes_for_max) { pevit_set_error("predict: workspace too small (%zu < %zu)", c->ws_bytes_for_max, c->lay.total); return -1; }
    StepPlan pl = plan_step(c, B, infer);
    pl.segments = segments;
    char* W = c->ws; char* A = c->arena;
    const int E = c->E, N = c->N, T = B * N;
    float* xpre = at<float>(W, c->lay.w_dxn);               // scratch, free during the forward pass
    if (u8) {
        Im2colU8Args a;
        a.img = (const unsigned char*)images_any; a.mean3 = c->img_mean; a.std3 = c->img_std; a.out = at<bf16>(W, c->lay.w_patches);
        a.B = B; a.R = c->R; a.P = c->P; a.Kp = c->Kpatch; a.f32 = c->f32;
        PROF(c, s, PEVIT_PROF_IM2COL, B, (double)B * 3 * c->R * c->R * 1 + (double)B * c->G2 * c->Kpatch * c->es, pevit_launch_im2col_u8(a, s));
    } else
        PROF(c, s, PEVIT_PROF_IM2COL, B, (double)B * 3 * c->R * c->R * 4 + (double)B * c->G2 * c->Kpatch * c->es,
             pevit_launch_im2col(images, at<bf16>(W, c->lay.w_patches), B, c->R, c->P, c->Kpatch, s, c->f32));
    CHECK(pevit_launch_cls_row(at<float>(A, c->a_cls), at<float>(A, c->a_pos), xpre, B, N, E, s));
    {
        GemmParams p = gp(at<bf16>(W, c->lay.w_patches), c->Kpatch, at<bf16>(A, c->a_conv), c->Kpatch, E, B * c->G2, E, c->Kpatch);
        p.resid = at<float>(A, c->a_pos); p.ldr = E; p.outf = xpre; p.ldo = E; p.Ntok = N;
        CHECK(gemm(c, EPI_PATCH_EMBED, p, s));
    }
    {
        LnFwdArgs a;     // ln_pre: f32 out, no statistics kept (nothing below the first block is trainable)
        a.x = xpre; a.gamma = at<float>(A, c->a_lnpre_w); a.beta = at<float>(A, c->a_lnpre_b); a.rows = T; a.E = E;
        a.y_f32 = at<float>(W, c->lay.sav[0].x_in);
        CHECK(pevit_launch_ln_fwd(a, s));
    }
    if (gate) {                                         // fused step with a gate (pevit_set_step_gate): parameters and gradient buffer from here on
        HIP_OK(hipStreamWaitEvent(s, c->step_gate, 0));
        CHECK(pevit_zero_grads(c, stream));
    }
    CHECK(blocks_forward(c, s, B, pl, pl.cls_prune));
    // ln_post on the class token of every image (row b*N), then @ proj
    {
        LnFwdArgs a;
        a.x = at<float>(W, c->lay.w_xfinal); a.gamma = at<float>(A, c->a_lnpost_w); a.beta = at<float>(A, c->a_lnpost_b); a.rows = B; a.E = E;
        a.y_bf16 = at<bf16>(W, c->lay.w_xpost);
        if (!infer) { a.mean = at<float>(W, c->lay.w_pmean); a.rstd = at<float>(W, c->lay.w_prstd); }
        a.xstride = (size_t)N * E; a.f32 = c->f32;
        CHECK(pevit_launch_ln_fwd(a, s));
    }
    {
        GemmParams p = gp(at<bf16>(W, c->lay.w_xpost), E, at<bf16>(A, c->a_proj), E, c->D, B, c->D, E);
        p.outf = feat ? feat : at<float>(W, c->lay.w_feat); p.ldo = c->D;
        CHECK(gemm(c, EPI_F32, p, s));
    }
    c->saved = infer ? SavedForward{} : SavedForward{Saved::visual, save_for_backward ? B : 0, -1, pl};
    return 0;
}
extern "C" int pevit_visual_forward(pevit_ctx* c, void* stream, const float* images, float* feat, int B,
                                    int save_for_backward) {
    CHECK(refuse_infer(c, "visual_forward"));
    return visual_forward_impl(c, stream, images, 0, feat, B, save_for_backward, false, false);
}
// the same from uint8 pixels (B,3,R,R): the reference's ToTensor + Normalize run inside the patch gather (pevit_set_input_norm)
extern "C" int pevit_visual_forward_u8(pevit_ctx* c, void* stream, const uint8_t* images, float* feat, int B,
                                       int save_for_backward) {
    CHECK(refuse_infer(c, "visual_forward_u8"));
    CHECK(check_u8_input(c, "visual_forward_u8"));
    return visual_forward_impl(c, stream, images, 1, feat, B, save_for_backward, false, false);
}

// images (B,3,R,R) -> logits (B,C) in ONE call, for evaluation: stem -> blocks -> ln_post -> proj in the inference form (blocks_forward,
// pl.infer), then BatchNorm1d in eval mode on the caller's running statistics -> Linear: the forward-only launch of pevit_launch_head.
// Reads parameters and running statistics, writes logits (and feat_or_null (B,D)) and workspace scratch only: not the gradient
// buffer, not last_loss.  batch 1 is legal (eval-mode BatchNorm takes no batch statistics).
static int predict_impl(pevit_ctx* c, void* stream, const void* images, int u8, const float* running_mean, const float* running_var,
                        float* logits, float* feat_or_null, int B) {
    CHECK(refuse_text(c, "predict"));
    CHECK(check_ready(c, B, "predict"));
    if (!c->params) { pevit_set_error("predict: parameters not set (the Linear head lives in the flat parameter buffer)"); return -1; }
    if (!images || !running_mean || !running_var || !logits) { pevit_set_error("predict: null argument"); return -1; }
    CHECK(visual_forward_impl(c, stream, images, u8, feat_or_null, B, 0, true, false));
    char* W = c->ws;
    HeadArgs a;
    a.feat = feat_or_null ? feat_or_null : at<float>(W, c->lay.w_feat); a.W = c->params + c->p_head_w; a.bias = c->params + c->p_head_b;
    // (training = 0: bn_fwd_kernel only reads the running statistics)
    a.running_mean = const_cast<float*>(running_mean); a.running_var = const_cast<float*>(running_var); a.training = 0;
    a.ybn = at<float>(W, c->lay.w_ybn); a.rstd = at<float>(W, c->lay.w_bnrstd); a.logits = logits; a.B = B; a.D = c->D; a.Cc = c->C;
    // (the forward-only launch touches neither; an inference-only context has no slot for them)
    if (!c->infer_only) { a.dlogits = at<float>(W, c->lay.w_dlogits); a.dybn = at<float>(W, c->lay.w_dybn); }
    return pevit_launch_head(a, (hipStream_t)stream);
}
extern "C" int pevit_predict(pevit_ctx* c, void* stream, const float* images, const float* running_mean, const float* running_var,
                             float* logits, float* feat_or_null, int B) {
    return predict_impl(c, stream, images, 0, running_mean, running_var, logits, feat_or_null, B);
}
extern "C" int pevit_predict_u8(pevit_ctx* c, void* stream, const uint8_t* images, const float* running_mean, const float* running_var,
                                float* logits, float* feat_or_null, int B) {
    CHECK(check_u8_input(c, "predict_u8"));
    return predict_impl(c, stream, images, 1, running_mean, running_var, logits, feat_or_null, B);
}

// Requests for several resident adapters in ONE walk (include/pevit_segments.h): everything but the attention site runs once on all B
// images, the attention site per segment on its slot's panels (walk.hip attn_core_fwd_slots), and the head once per segment on the
// segment's feature rows with the slot's Linear layer and the segment's running statistics.  Every refusal comes before any launch.
static int predict_segments_impl(pevit_ctx* c, void* stream, const void* images, int u8, int B, int nseg, const pevit_segment* segs) {
    const char* who = "predict_segments";
    CHECK(refuse_text(c, who));
    if (!c || !c->arena || !c->ws) { pevit_set_error("%s: context not bound", who); return -1; }
    if (!c->slots) { pevit_set_error("%s: this context has no adapter slots (pevit_infer_create_slots)", who); return -1; }
    if (!images || !segs) { pevit_set_error("%s: null argument", who); return -1; }
    if (B <= 0 || B > c->max_batch) { pevit_set_error("%s: batch %d outside [1,%d]", who, B, c->max_batch); return -1; }
    if (nseg < 1 || nseg > PEVIT_MAX_SEGMENTS_PER_CALL) { pevit_set_error("%s: %d segments outside [1,%d]", who, nseg, PEVIT_MAX_SEGMENTS_PER_CALL); return -1; }
    int next = 0;
    for (int i = 0; i < nseg; ++i) {
        const pevit_segment& g = segs[i];
        if (g.first != next || g.count < 1 || g.count > B - next) {
            pevit_set_error("%s: segment %d is images [%d, %d): the segments must tile [0, %d) in order, one image at least each", who, i,
                            g.first, g.first + g.count, B);
            return -1;
        }
        if (g.slot < 0 || g.slot >= c->slots) { pevit_set_error("%s: segment %d names slot %d outside [0,%d)", who, i, g.slot, c->slots); return -1; }
        if (!c->slot_params[g.slot]) { pevit_set_error("%s: segment %d names slot %d, which is not loaded (pevit_load_adapter_slot)", who, i, g.slot); return -1; }
        if (!g.running_mean || !g.running_var || !g.logits) { pevit_set_error("%s: segment %d: null argument", who, i); return -1; }
        next += g.count;
    }
    if (next != B) { pevit_set_error("%s: the segments cover %d of %d images: they must tile [0, %d)", who, next, B, B); return -1; }
    c->nseg = nseg;
    for (int i = 0; i < nseg; ++i) c->segs[i] = segs[i];
    hipStream_t s = (hipStream_t)stream;
    CHECK(visual_forward_impl(c, stream, images, u8, nullptr, B, 0, true, false, true));
    char* W = c->ws;
    const float* feat = at<float>(W, c->lay.w_feat);
    for (int i = 0; i < nseg; ++i) {
        const pevit_segment& g = segs[i];
        const float* p = c->slot_params[g.slot];
        const int Cs = c->slot_classes[g.slot];
        HeadArgs a;
        a.feat = feat + (size_t)g.first * c->D; a.W = p + c->n_tower; a.bias = a.W + (size_t)Cs * c->D;
        a.running_mean = const_cast<float*>(g.running_mean); a.running_var = const_cast<float*>(g.running_var); a.training = 0;
        a.ybn = at<float>(W, c->lay.w_ybn); a.rstd = at<float>(W, c->lay.w_bnrstd); a.logits = g.logits; a.B = g.count; a.D = c->D; a.Cc = Cs;
        CHECK(pevit_launch_head(a, s));
        if (g.features) HIP_OK(hipMemcpyAsync(g.features, a.feat, (size_t)g.count * c->D * 4, hipMemcpyDeviceToDevice, s));
    }
    return 0;
}
extern "C" int pevit_predict_segments(pevit_ctx* c, void* stream, const float* images, int B, int nseg, const pevit_segment* segs) {
    return predict_segments_impl(c, stream, images, 0, B, nseg, segs);
}
extern "C" int pevit_predict_segments_u8(pevit_ctx* c, void* stream, const uint8_t* images, int B, int nseg, const pevit_segment* segs) {
    CHECK(check_u8_input(c, "predict_segments_u8"));
    return predict_segments_impl(c, stream, images, 1, B, nseg, segs);
}

// images (B,3,R,R) -> features (B,D) through the inference forms, without a head (CLIP.encode_image for evaluation).  Like
// pevit_predict it leaves no saved forward behind.
static int encode_image_impl(pevit_ctx* c, void* stream, const void* images, int u8, float* feat, int B) {
    CHECK(refuse_text(c, "encode_image"));
    CHECK(check_ready(c, B, "encode_image"));
    if (!images || !feat) { pevit_set_error("encode_image: null argument"); return -1; }
    return visual_forward_impl(c, stream, images, u8, feat, B, 0, true, false);
}
extern "C" int pevit_encode_image(pevit_ctx* c, void* stream, const float* images, float* feat, int B) {
    return encode_image_impl(c, stream, images, 0, feat, B);
}
extern "C" int pevit_encode_image_u8(pevit_ctx* c, void* stream, const uint8_t* images, float* feat, int B) {
    CHECK(check_u8_input(c, "encode_image_u8"));
    return encode_image_impl(c, stream, images, 1, feat, B);
}

// images (B,3,R,R) -> zero-shot class probabilities (B x num_classes) in one call: the same walk, then the cosine head and its
// softmax in one launch (zeroshot.hip) on the features.  text_cd: (num_classes x D) f32, one unit vector per class; num_classes is
// independent of pevit_dims.num_classes.  The head's limits are checked before the tower runs.
static int zeroshot_impl(pevit_ctx* c, void* stream, const void* images, int u8, const float* text_cd, int num_classes, float scale,
                         float* probs, float* logits, float* feat_or_null, int B) {
    CHECK(refuse_text(c, "zeroshot"));
    CHECK(check_ready(c, B, "zeroshot"));
    if (!images) { pevit_set_error("zeroshot: null argument"); return -1; }
    ZeroshotArgs a;
    a.feat = feat_or_null ? feat_or_null : at<float>(c->ws, 0);     // (for the check: the w_feat slot is known after the walk)
    a.text = text_cd; a.scale = scale; a.probs = probs; a.logits = logits; a.B = B; a.D = c->D; a.C = num_classes;
    CHECK(pevit_zeroshot_check(a));
    CHECK(visual_forward_impl(c, stream, images, u8, feat_or_null, B, 0, true, false));
    a.feat = feat_or_null ? feat_or_null : at<float>(c->ws, c->lay.w_feat);
    return pevit_launch_zeroshot_head(a, (hipStream_t)stream);
}
extern "C" int pevit_zeroshot(pevit_ctx* c, void* stream, const float* images, const float* text_cd, int num_classes, float scale,
                              float* probs_or_null, float* logits_or_null, float* feat_or_null, int B) {
    return zeroshot_impl(c, stream, images, 0, text_cd, num_classes, scale, probs_or_null, logits_or_null, feat_or_null, B);
}
extern "C" int pevit_zeroshot_u8(pevit_ctx* c, void* stream, const uint8_t* images, const float* text_cd, int num_classes, float scale,
                                 float* probs_or_null, float* logits_or_null, float* feat_or_null, int B) {
    CHECK(check_u8_input(c, "zeroshot_u8"));
    return zeroshot_impl(c, stream, images, 1, text_cd, num_classes, scale, probs_or_null, logits_or_null, feat_or_null, B);
}

// ---- the linear probe on cached feature rows (probe.hip): context checks in the order a caller can meet them without a device
static int probe_check_ctx(const pevit_ctx* c, const char* who) {
    if (!c) { pevit_set_error("%s: null context", who); return -1; }
    CHECK(refuse_text(c, who));
    CHECK(refuse_infer(c, who));
    if (c->d.method != PEVIT_NONE) {
        pevit_set_error("%s: the context's method is not PEVIT_NONE (the probe trains the head over a frozen tower; the adapter "
                        "methods train through pevit_train_forward_backward)", who);
        return -1;
    }
    return pevit_probe_check(c->D, c->C, who);
}
static int probe_check_bound(const pevit_ctx* c, const char* who) {
    if (!c->arena || !c->ws) { pevit_set_error("%s: context not bound", who); return -1; }
    if (!c->params || !c->grads || !c->mom) { pevit_set_error("%s: parameters not set (pevit_set_params)", who); return -1; }
    return 0;
}
extern "C" int pevit_probe_step(pevit_ctx* c, void* stream, const pevit_probe_args* p) {
    CHECK(probe_check_ctx(c, "probe_step"));
    if (!p) { pevit_set_error("probe_step: null argument struct"); return -1; }
    // torch.nn.BatchNorm1d refuses one value per channel in training mode and the reference's train_one skips such batches
    // (full_model_finetune.py:316); the harness skips them too, so a batch of one is a caller's mistake in either mode
    if (p->batch < 2) { pevit_set_error("probe_step: batch %d must be at least 2", p->batch); return -1; }
    CHECK(probe_check_bound(c, "probe_step"));
    if (p->batch > c->max_batch) { pevit_set_error("probe_step: batch %d exceeds max_batch %d of the bound workspace", p->batch, c->max_batch); return -1; }
    if (!p->feat || !p->index || !p->running_mean || !p->running_var || !p->logits || !p->loss) { pevit_set_error("probe_step: null argument"); return -1; }
    if (!p->labels == !p->targets) { pevit_set_error("probe_step: exactly one of labels and targets must be given"); return -1; }
    if (p->rows < 1) { pevit_set_error("probe_step: %lld feature rows (at least 1)", (long long)p->rows); return -1; }
    if (p->rows > 0x7fffffffLL) { pevit_set_error("probe_step: %lld feature rows (at most 2^31 - 1)", (long long)p->rows); return -1; }
    if (reinterpret_cast<size_t>(p->feat) & 15) { pevit_set_error("probe_step: feat must be 16-byte aligned"); return -1; }
    c->saved = SavedForward{};                    // the head slots of the workspace are laid out for THIS batch
    c->lay = layout_workspace(c, p->batch);
    char* W = c->ws;
    ProbeArgs a;
    a.feat = p->feat; a.index = p->index; a.labels = p->labels; a.targets = p->targets; a.rows = (long)p->rows;
    a.W = a.pW = c->params + c->p_head_w; a.bias = a.pB = c->params + c->p_head_b;
    a.gW = c->grads + c->p_head_w; a.gB = c->grads + c->p_head_b; a.mW = c->mom + c->p_head_w; a.mB = c->mom + c->p_head_b;
    a.running_mean = p->running_mean; a.running_var = p->running_var;
    a.xhat = at<float>(W, c->lay.w_ybn); a.dlogits = at<float>(W, c->lay.w_dlogits); a.rowloss = at<float>(W, c->lay.w_dybn);
    a.logits = p->logits; a.loss = p->loss;
    a.B = p->batch; a.D = c->D; a.C = c->C; a.training = p->bn_training != 0; a.update = p->update != 0; a.flags = p->flags;
    a.scale = p->scale; a.lr = p->lr; a.momentum = p->momentum; a.wd = p->weight_decay;
    c->last_loss = a.update ? nullptr : p->loss;     // (a following pevit_optim_step writes NaN there when an error word withholds it)
    return pevit_launch_probe_step(a, (hipStream_t)stream);
}
extern "C" int pevit_probe_predict(pevit_ctx* c, void* stream, const pevit_probe_predict_args* p) {
    CHECK(probe_check_ctx(c, "probe_predict"));
    if (!p) { pevit_set_error("probe_predict: null argument struct"); return -1; }
    if (p->count < 1) { pevit_set_error("probe_predict: %d rows (at least 1)", p->count); return -1; }
    CHECK(probe_check_bound(c, "probe_predict"));
    if (!p->feat || !p->running_mean || !p->running_var || !p->logits) { pevit_set_error("probe_predict: null argument"); return -1; }
    if (p->rows < 1) { pevit_set_error("probe_predict: %lld feature rows (at least 1)", (long long)p->rows); return -1; }
    if (!p->index_or_null && (p->first_row < 0 || p->first_row + p->count > p->rows)) {
        pevit_set_error("probe_predict: rows [%lld, %lld) outside the %lld feature rows", (long long)p->first_row,
                        (long long)(p->first_row + p->count), (long long)p->rows);
        return -1;
    }
    if (p->rows > 0x7fffffffLL) { pevit_set_error("probe_predict: %lld feature rows (at most 2^31 - 1)", (long long)p->rows); return -1; }
    if (reinterpret_cast<size_t>(p->feat) & 15) { pevit_set_error("probe_predict: feat must be 16-byte aligned"); return -1; }
    ProbeArgs a;
    a.feat = p->feat; a.index = p->index_or_null; a.rows = (long)p->rows; a.row0 = (long)p->first_row;
    a.W = c->params + c->p_head_w; a.bias = c->params + c->p_head_b;
    a.running_mean = const_cast<float*>(p->running_mean); a.running_var = const_cast<float*>(p->running_var);
    a.logits = p->logits; a.B = p->count; a.D = c->D; a.C = c->C; a.scale = p->scale;
    return pevit_launch_probe_predict(a, (hipStream_t)stream);
}

// tokens (S,N) int64 -> features (S,D) f32                              model.py:1153-1168
extern "C" int pevit_encode_text(pevit_ctx* c, void* stream, const int64_t* tokens, float* features, int S) {
    CHECK(refuse_infer(c, "encode_text"));
    if (c && !c->text) { pevit_set_error("encode_text: this is an image context (pevit_ctx_create); text contexts come from pevit_text_create"); return -1; }
    CHECK(check_ready(c, S, "encode_text"));
    if (!tokens || !features) { pevit_set_error("encode_text: null argument"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    c->saved = SavedForward{};
    c->lay = layout_workspace(c, S, true);
    if (c->lay.total > c->ws_bytes_for_max) { pevit_set_error("encode_text: workspace too small (%zu < %zu)", c->ws_bytes_for_max, c->lay.total); return -1; }
    const StepPlan pl = plan_step(c, S, true);
    char* W = c->ws; char* A = c->arena;
    const int E = c->E, N = c->N;
    {
        TextEmbedArgs a;     // straight into the first block's input slot
        a.tokens = tokens; a.table = at<float>(A, c->a_tok); a.pos = at<float>(A, c->a_pos); a.x = at<float>(W, c->lay.sav[0].x_in);
        a.S = S; a.N = N; a.E = E; a.V = c->V;
        CHECK(pevit_launch_text_embed(a, s));
    }
    CHECK(blocks_forward(c, s, S, pl, false));
    // the end-of-text row of every prompt -> ln_final -> @ text_projection
    float* eot = at<float>(W, c->lay.w_dxn);                // [S][E] f32 scratch (free in a forward pass)
    CHECK(pevit_launch_text_eot_gather(tokens, at<float>(W, c->lay.w_xfinal), eot, S, N, E, s));
    {
        LnFwdArgs a;
        a.x = eot; a.gamma = at<float>(A, c->a_lnpost_w); a.beta = at<float>(A, c->a_lnpost_b); a.rows = S; a.E = E;
        a.y_bf16 = at<bf16>(W, c->lay.w_xpost); a.f32 = c->f32;
        CHECK(pevit_launch_ln_fwd(a, s));
    }
    {
        GemmParams p = gp(at<bf16>(W, c->lay.w_xpost), E, at<bf16>(A, c->a_proj), E, c->D, S, c->D, E);
        p.outf = features; p.ldo = c->D;
        CHECK(gemm(c, EPI_F32, p, s));
    }
    return 0;
}

// dfeat (B,D) f32 -> adapter gradients (nothing below the first block is trainable).
// Layers l_hi-1 .. l_lo; the entry work (proj^T, ln_post backward) belongs to the part that starts at L.  Data
// parallelism calls (L, L/2) then (L/2, 0) and all-reduces the first part's gradients while the second runs.
extern "C" int pevit_visual_backward_part(pevit_ctx* c, void* stream, const float* dfeat, int B, int l_hi, int l_lo) {
    CHECK(refuse_text(c, "visual_backward"));
    CHECK(refuse_infer(c, "visual_backward"));
    CHECK(check_ready(c, B, "visual_backward"));
    CHECK(check_saved(c, Saved::visual, B, -1, "visual_backward"));
    CHECK(check_range(c, l_lo, l_hi, "visual_backward", "layer"));
    if (c->d.method == PEVIT_NONE) return 0;
    hipStream_t s = (hipStream_t)stream;
    char* W = c->ws; char* A = c->arena;
    const int E = c->E, N = c->N, T = B * N;
    const StepPlan& pl = c->saved.plan;
    const bool cls = pl.cls_prune;
    if (l_hi == c->L) {
        if (!dfeat) { pevit_set_error("visual_backward: dfeat is required for the part that starts at the last block"); return -1; }
        // (the head's BatchNorm backward leaves the bf16 copy of ITS dfeat in w_dfeatb: no cast launch then)
        if (c->dfeatb_of != dfeat) CHECK(pevit_launch_cast_bf16(dfeat, at<bf16>(W, c->lay.w_dfeatb), (size_t)B * c->D, 1.0f, s, c->f32));
        c->dfeatb_of = nullptr;
        {
            GemmParams p = gp(at<bf16>(W, c->lay.w_dfeatb), c->D, at<bf16>(A, c->a_projT), c->D, E, B, E, c->D);
            p.outf = at<float>(W, c->lay.w_dxpost); p.ldo = E;
            CHECK(gemm(c, EPI_F32, p, s));
        }
        // dL/dx_final is zero except on the class-token rows.  With class-token pruning of the last block
        // only those rows of dxa / dyb are ever read; the full-size buffers the last block's attention and
        // LN1 backward consume (dO, dxb) are zeroed instead.
        if (cls) {
            // ... or not read at all: LayerNorm backward takes the residual gradient on the class-token rows only (res_period), and
            // the attention backward for N <= 64 reads dO on token 0 only (dout_cls_only) -- no fill of dxb (19.7 MB) / dO (9.8 MB)
            if (c->f32 || N > 64) CHECK(pevit_launch_zero(W + c->lay.w_dO, (size_t)T * E * c->es, s));
        } else {
            if (!pl.gstream16) CHECK(pevit_launch_zero(W + c->lay.w_dxa, (size_t)T * E * 4, s));      // (the bf16 stream never reads the f32 copy)
            CHECK(pevit_launch_zero(W + c->lay.w_dyb, (size_t)T * E * c->es, s));
        }
        LnBwdArgs a;     // ln_post backward on the class-token rows: no residual gradient joins here
        a.dy = at<float>(W, c->lay.w_dxpost); a.x = at<float>(W, c->lay.w_xfinal); a.mean = at<float>(W, c->lay.w_pmean);
        a.rstd = at<float>(W, c->lay.w_prstd); a.gamma = at<float>(A, c->a_lnpost_w); a.dx_out = at<float>(W, c->lay.w_dxa);
        a.dx_bf16 = at<bf16>(W, c->lay.w_dyb); a.rows = B; a.E = E; a.xstride = (size_t)N * E; a.f32 = c->f32;
        if (c->fp8) a.bf16_colscale = at<float>(A, c->blk[c->L - 1].spr);
        CHECK(pevit_launch_ln_bwd(a, s));
    }
    CHECK(blocks_backward(c, s, B, pl, false, cls, l_hi, l_lo));
    return 0;
}

extern "C" int pevit_visual_backward(pevit_ctx* c, void* stream, const float* dfeat, int B) {
    return pevit_visual_backward_part(c, stream, dfeat, B, c ? c->L : 0, 0);
}

// labels (B) int64 -> cross-entropy, targets (B x C) f32 -> BCE with logits, neither -> forward only; never both
// fused_step: the caller is train_fb_impl, where nobody can touch dfeat between the head and the tower backward
static int head_fb_impl(pevit_ctx* c, void* stream, const float* feat, const int64_t* labels, const float* targets,
                        float* running_mean, float* running_var, int bn_training, float* logits, float* loss, float* dfeat, int B,
                        bool fused_step) {
    CHECK(refuse_text(c, "head_forward_backward"));
    CHECK(refuse_infer(c, "head_forward_backward"));
    if (!c || !c->ws || !c->params || !c->grads) { pevit_set_error("head: context not ready"); return -1; }
    if (B <= 0 || B > c->max_batch) { pevit_set_error("head: batch %d outside [1,%d]", B, c->max_batch); return -1; }
    if (!feat || !running_mean || !running_var || !logits) { pevit_set_error("head: null argument"); return -1; }
    if (labels && targets) { pevit_set_error("head: labels and targets both given"); return -1; }
    const bool has_loss = labels || targets;
    if (has_loss && !loss) { pevit_set_error("head: labels given but loss is null"); return -1; }
    // torch.nn.BatchNorm1d raises "Expected more than 1 value per channel when training" (the reference's train_one
    // skips such batches, kadaptation_clip.py:341); the batch variance of one sample is 0, never a usable statistic
    if (bn_training && B < 2) { pevit_set_error("head: BatchNorm in training mode needs more than 1 sample per batch (got %d)", B); return -1; }
    hipStream_t s = (hipStream_t)stream;
    char* W = c->ws;
    // the head slots of the layout a saving forward left serve every batch up to that forward's; a larger one would overrun
    // them into each other (ybn into rstd, dlogits, dybn ...): lay the workspace out for THIS batch, which gives the saved
    // activations up -- check_saved refuses a backward through them from here on
    if (B > c->saved.batch) { c->saved.batch = 0; c->lay = layout_workspace(c, B); }
    if (has_loss) c->last_loss = loss;
    // only inside the fused step: the head's BatchNorm backward leaves the bf16 copy of dfeat for the tower backward
    bf16* dfb = (fused_step && dfeat && has_loss && !c->f32) ? at<bf16>(W, c->lay.w_dfeatb) : nullptr;
    c->dfeatb_of = dfb ? dfeat : nullptr;
    HeadArgs a;
    a.feat = feat; a.labels = labels; a.targets = targets; a.W = c->params + c->p_head_w; a.bias = c->params + c->p_head_b;
    if (has_loss) { a.gW = c->grads + c->p_head_w; a.gb = c->grads + c->p_head_b; }
    a.running_mean = running_mean; a.running_var = running_var; a.training = bn_training;
    a.ybn = at<float>(W, c->lay.w_ybn); a.rstd = at<float>(W, c->lay.w_bnrstd); a.logits = logits; a.dlogits = at<float>(W, c->lay.w_dlogits);
    a.dybn = at<float>(W, c->lay.w_dybn); a.loss = loss; a.dfeat = dfeat; a.B = B; a.D = c->D; a.Cc = c->C; a.dfeat_bf16 = dfb;
    return pevit_launch_head(a, s);
}
extern "C" int pevit_head_forward_backward(pevit_ctx* c, void* stream, const float* feat, const int64_t* labels,
                                           float* running_mean, float* running_var, int bn_training, float* logits,
                                           float* loss, float* dfeat, int B) {
    return head_fb_impl(c, stream, feat, labels, nullptr, running_mean, running_var, bn_training, logits, loss, dfeat, B, false);
}
extern "C" int pevit_head_forward_backward_bce(pevit_ctx* c, void* stream, const float* feat, const float* targets,
                                               float* running_mean, float* running_var, int bn_training, float* logits,
                                               float* loss, float* dfeat, int B) {
    CHECK(refuse_text(c, "head_forward_backward_bce"));
    CHECK(refuse_infer(c, "head_forward_backward_bce"));
    if (!targets) { pevit_set_error("head_bce: targets is null (the forward alone is pevit_head_forward_backward with no labels)"); return -1; }
    return head_fb_impl(c, stream, feat, nullptr, targets, running_mean, running_var, bn_training, logits, loss, dfeat, B, false);
}

static int train_fb_impl(pevit_ctx* c, void* stream, const void* images, int u8, const int64_t* labels, const float* targets,
                         float* running_mean, float* running_var, int bn_training, float* logits, float* loss, int B) {
    CHECK(refuse_text(c, "train_forward_backward"));
    CHECK(refuse_infer(c, "train_forward_backward"));
    CHECK(check_ready(c, B, "train_forward_backward"));
    if (!labels == !targets) { pevit_set_error("train_forward_backward: exactly one of labels and targets must be given"); return -1; }
    const bool gate = c->step_gate != nullptr;          // with a gate the gradients are cleared behind it, inside the forward pass
    if (!gate) CHECK(pevit_zero_grads(c, stream));
    CHECK(visual_forward_impl(c, stream, images, u8, nullptr, B, 1, false, gate));
    float* feat = at<float>(c->ws, c->lay.w_feat);
    float* dfeat = at<float>(c->ws, c->lay.w_dfeat);
    const int hrc = head_fb_impl(c, stream, feat, labels, targets, running_mean, running_var, bn_training, logits, loss, dfeat, B, true);
    if (hrc) { c->dfeatb_of = nullptr; return hrc; }
    CHECK(pevit_visual_backward(c, stream, dfeat, B));
    return 0;
}
extern "C" int pevit_train_forward_backward(pevit_ctx* c, void* stream, const float* images, const int64_t* labels,
                                            float* running_mean, float* running_var, int bn_training, float* logits,
                                            float* loss, int B) {
    return train_fb_impl(c, stream, images, 0, labels, nullptr, running_mean, running_var, bn_training, logits, loss, B);
}
extern "C" int pevit_train_forward_backward_u8(pevit_ctx* c, void* stream, const uint8_t* images, const int64_t* labels,
                                               float* running_mean, float* running_var, int bn_training, float* logits,
                                               float* loss, int B) {
    CHECK(refuse_infer(c, "train_forward_backward_u8"));
    CHECK(check_u8_input(c, "train_forward_backward_u8"));
    return train_fb_impl(c, stream, images, 1, labels, nullptr, running_mean, running_var, bn_training, logits, loss, B);
}
extern "C" int pevit_train_forward_backward_bce(pevit_ctx* c, void* stream, const float* images, const float* targets,
                                                float* running_mean, float* running_var, int bn_training, float* logits,
                                                float* loss, int B) {
    return train_fb_impl(c, stream, images, 0, nullptr, targets, running_mean, running_var, bn_training, logits, loss, B);
}
extern "C" int pevit_train_forward_backward_bce_u8(pevit_ctx* c, void* stream, const uint8_t* images, const float* targets,
                                                   float* running_mean, float* running_var, int bn_training, float* logits,
                                                   float* loss, int B) {
    CHECK(refuse_infer(c, "train_forward_backward_bce_u8"));
    CHECK(check_u8_input(c, "train_forward_backward_bce_u8"));
    return train_fb_impl(c, stream, images, 1, nullptr, targets, running_mean, running_var, bn_training, logits, loss, B);
}

// 1 if a stream-K consumer ever gave up waiting for a partial tile (context-free workspace when ctx is null); clears it
extern "C" int pevit_streamk_error(pevit_ctx* c, void* stream) {
    GemmParams p; memset(&p, 0, sizeof(p));
    unsigned* flag = nullptr;
    if (c) { if (!c->ws || !c->sk_slots) return 0; flag = at<unsigned>(c->ws, c->lay.w_skflag) + c->sk_slots; }
    else { if (op_sk_workspace(p)) return -1; flag = p.sk_flag + p.sk_slots; }
    unsigned v = 0;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return -1;
    if (hipMemcpy(&v, flag, 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (v) {
        (void)hipMemset(flag, 0, 4);
        if (c) (void)hipMemset(at<unsigned>(c->ws, c->lay.w_skflag) + PEVIT_SK_MAX_SLOTS + 1, 0, 4);    // the skipped-update counter with it
    }
    return v ? 1 : 0;
}
// the same word without clearing it, plus the number of optimizer updates the fused SGD kernel withheld because of it.  A caller
// that wants to go on after the error calls pevit_streamk_error (which clears the word) and knows how many steps it lost.
extern "C" int pevit_streamk_status(pevit_ctx* c, void* stream, unsigned* error_word, unsigned* skipped_updates) {
    if (!c) { pevit_set_error("streamk_status: null context"); return -1; }
    unsigned v[2] = {0, 0};
    if (c->ws && c->sk_slots) {
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return -1;
        if (hipMemcpy(&v[0], at<unsigned>(c->ws, c->lay.w_skflag) + c->sk_slots, 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
        if (hipMemcpy(&v[1], at<unsigned>(c->ws, c->lay.w_skflag) + PEVIT_SK_MAX_SLOTS + 1, 4, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    }
    if (error_word) *error_word = v[0];
    if (skipped_updates) *skipped_updates = v[1];
    return 0;
}
