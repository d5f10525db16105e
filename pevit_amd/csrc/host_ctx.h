// The host side of the engine, private to csrc/: the context, the memory layout of the weight arena / workspace, the plan of a step,
// and what ctx.hip, profile.hip, walk.hip and step.hip call in each other.  ops.hip (the context-free pevit_op_* test seams) does not
// include this header.  See include/pevit_hip.h for the boundary contract.
#pragma once
#include <string.h>

#include <vector>

#include "../../include/pevit_hip.h"
#include "common.h"
#include "kernels.h"

#define CHECK(call)            \
    do {                       \
        if ((call) != 0) return -1; \
    } while (0)

// everything the units share lives in this namespace; hidden, so that the library exports the C ABI and the launchers as before
namespace pevit_host __attribute__((visibility("hidden"))) {

// the head of every workspace layout, the only part that carries state between launches (pevit_workspace_state_bytes): the
// stream-K hand-off flags + the error word + the skipped-update counter
constexpr size_t WS_STATE_BYTES = (size_t)(PEVIT_SK_MAX_SLOTS + 2) * 4;

struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    }
};

struct BlockArena {        // byte offsets inside the weight arena, one per layer
    size_t wqkv, wqkvT, wo, woT, wfc, wfcT, wpr, wprT;
    size_t bqkv, bo, bfc, bpr, ln1w, ln1b, ln2w, ln2b;
    size_t q32, qT, q16;
    size_t wd, wdT, wu, wuT;      // post-MLP adapter panels (bf16), rewritten every step
    size_t wpan;                  // fp8 weights only: the 64 adapter rows P_q^T | P_v^T (bf16) of the separate t = xn P product
    size_t sqkv, so, sfc, spr;    // fp8 weights only: per-output-channel scales (f32, powers of two)
    size_t tsink;                 // inference-only contexts: [E][64] write-only panel that takes the transposed stores of the prep kernels
    size_t q16s;                  // multi-slot contexts: the [E][64] bf16 Q panels of the slots, q16_slot_bytes apart (q16: the single-adapter calls')
    size_t wds, wus;              // post-MLP slot contexts: the [64][E] down / [E][64] up bf16 panels of the slots, pm_slot_bytes apart (wd, wu: the single-adapter calls')
};

struct LayerSaved {        // byte offsets inside the workspace, one per layer (kept for backward)
    size_t x_in, x_mid, mean1, rstd1, mean2, rstd2, xn1, qkv, t, lse, attn_out, h;
    size_t hf32, mean_a, rstd_a, z, apre, act;     // post-MLP adapters
};

struct WsLayout {          // byte offsets inside the workspace for one batch (layout_workspace)
    std::vector<LayerSaved> sav;
    size_t w_skflag, w_skslab;      // stream-K workspace (gemm_streamk.hip, gemm_skinny.hip, gemm_split.hip)
    size_t w_a8, w_attn8;           // e4m3 copies of the LayerNorm output / the attention output (fp8act)
    size_t w_xfinal, w_xn2, w_g, w_dqkv, w_u32, w_u32b, w_dO, w_dh, w_dxn, w_dxa, w_dxb, w_dyb, w_partial, w_dbias, w_G, w_rule;
    size_t w_dpre, w_dpre2, w_dht, w_dhb, w_tnU, w_tnD, w_csx, w_csy, w_lnp, w_Gd, w_Gu;
    size_t w_patches, w_xpost, w_feat, w_pmean, w_prstd, w_ybn, w_bnrstd, w_logits, w_dlogits, w_dybn, w_dfeat, w_dfeatb, w_dxpost;
    size_t partial_layer, dbias_layer, tn_layer, csx_layer, csy_layer, lnp_layer;    // per-layer slab strides
    size_t total;
};

// Every path choice of a step, made once by plan_step() when a forward starts and kept with its saved activations, so that a
// backward walks the paths its forward took: a knob changed in between takes effect at the next forward.
struct StepPlan {
    bool site = false;           // attention-site adapters (KAdaptation, LoRA): 64 adapter columns ride on the QKV product
    bool post_mlp = false;       // post-MLP adapters (Adapter, Compacter)
    bool cls_prune = false;      // visual tower: the last block after its attention core on the class-token rows only
    bool attn_delta = false;     // delta-add + attention forward as one launch (attn_delta.hip)
    bool fp8_tail = false;       // fp8 weights: t = xn P as the bf16 tail of the QKV launch where pevit_gemm_mixed_ok allows it
    bool adapter_fused = false;  // post-MLP adapter as one launch per direction (adapter_fused.hip)
    bool tn_fold = false;        // ... and both token-contracted weight-gradient products inside its backward launch
    int tn_fold_wgs = 0;         // ... on that many workgroups (0: the kernel's own count)
    bool gstream16 = false;      // the residual GRADIENT stream of the backward in bf16 only
    bool dx_stored = false;      // dX GEMMs hand the LN-input gradient to LayerNorm backward in the storage type
    bool lowrank_combo = false;  // u + dQ + d bias of a layer and the dP of the layer before it as one launch
    bool lowrank_xcd = false;    // lowrank_grad: XCD-contiguous workgroup order
    bool segments = false;       // segmented call (pevit_predict_segments): the attention site per segment on the slots' panels, no prep launch
    bool infer = false;          // inference walk (pevit_predict): the kernel forms that store nothing for a backward pass, one set of activation slots for all layers
};

// which forward the saved activations belong to
enum class Saved { none, blocks, visual, attention };
struct SavedForward {
    Saved kind = Saved::none;
    int batch = 0;               // 0: no backward may use them
    int layer = -1;              // attention seam: its layer
    StepPlan plan;               // the paths that forward took
};

// Cross-layer state of the attention-site adapter gradients over one backward walk (block walk or attention seam): the dP of the
// previously processed layer that lowrank_combo defers by one launch.
struct AttnGradWalk {
    int prev_layer = -1, u_par = 0;
    float* u_last = nullptr;
};

}  // namespace pevit_host

struct pevit_ctx {
    pevit_dims d;
    int E, L, H, N, P, R, D, C, G2, Kpatch;
    int NQ, NQpad;            // 3E+64 (multi-slot context: 3E + 64 (slots + 1)) and its multiple-of-128 padding
    bool fp8 = false;         // frozen block weights as e4m3 codes + per-channel scales (fp8.hip)
    bool fp8act = false;      // ... and fp8 A operands in the forward frozen products (PEVIT_W_FP8_ACT)
    bool f32 = false;         // f32-class verification mode: every bf16-declared buffer holds f32 (verify.hip)
    bool text = false;        // CLIP text tower (pevit_text_create): N = context_length, inference only, pevit_encode_text is its one forward
    bool causal = false;      // ... its attention is causal (attn_core_fwd passes this to the attention launch)
    bool infer_only = false;  // pevit_infer_create: no transposed weight copies, the third workspace layout, no gradients; runs the inference walk only
    // multi-slot context (pevit_infer_create_slots; 0: none).  Rows [3E + 64 s, + 64) of wqkv hold slot s's P rows, the rows behind
    // the last slot those of the single-adapter calls, which prep_adapters rebuilds per call: NQ = 3E + 64 (slots + 1) covers them,
    // a segmented call's product stops at 3E + 64 slots.
    // Post-MLP methods (pevit_infer_create_slots_all): `slots` counts the same, but nothing of the above grows (site_slots() is 0):
    // a slot is two panels per layer (BlockArena::wds, wus), and the workspace is that of pevit_infer_create
    int slots = 0;
    const float* slot_params[PEVIT_MAX_SLOTS] = {};     // pevit_load_adapter_slot: the flat buffer of each slot (null: not loaded) ...
    int slot_classes[PEVIT_MAX_SLOTS] = {};             // ... and its class count
    int nseg = 0;                                       // the segments of the segmented call in flight
    pevit_segment segs[PEVIT_MAX_SEGMENTS_PER_CALL] = {};
    int V = 0;                // ... vocabulary size (rows of the token-embedding table)
    size_t a_tok = 0;         // ... arena offset of the f32 token-embedding table [V][E]
    size_t es = 2;            // bytes per element of those buffers
    float ascale;             // 160 (model.py:564) or alpha/r (lora_model.py:491)
    // arena
    pevit_host::BlockArena* blk = nullptr;
    size_t a_conv, a_cls, a_pos, a_lnpre_w, a_lnpre_b, a_lnpost_w, a_lnpost_b, a_proj, a_projT, a_phm;
    size_t arena_bytes = 0;
    char* arena = nullptr;
    // workspace: the layout of the batch in flight
    pevit_host::WsLayout lay;
    int sk_slots = 0;         // stream-K slots (gemm_plan.h sk_slots), 0: disabled
    // post-MLP adapter parameter offsets inside one layer's block of the flat buffer (floats)
    size_t o_nw, o_nb, o_dw, o_db, o_uw, o_ub, o_dWl, o_dWr, o_uWl, o_uWr;
    size_t ws_bytes_for_max = 0;
    char* ws = nullptr;
    int max_batch = 0;
    // parameters
    float* params = nullptr; float* grads = nullptr; float* mom = nullptr;
    const unsigned char* grad_mask = nullptr;   // device, 1 = parameter receives gradients
    float* exp_avg_sq = nullptr;                // pevit_set_optim_state: Adam's second moment (exp_avg is `mom`) ...
    const unsigned char* group_of = nullptr;    // ... and every element's parameter group (255: no gradient)
    size_t n_tower = 0, n_total = 0;
    size_t p_layer0 = 0, p_layer_stride = 0;     // offsets in floats
    size_t p_head_w = 0, p_head_b = 0;
    float img_mean[3] = {0.f, 0.f, 0.f}, img_std[3] = {1.f, 1.f, 1.f};   // pevit_set_input_norm: preprocessing of uint8 pixels
    bool img_norm_set = false;
    pevit_host::SavedForward saved;
    // optional per-GEMM timing (HIP events on the caller's stream), see pevit_profile_begin
    bool prof_on = false;
    int prof_all = 0;         // also bracket the HBM-bound kernels (pevit_tune "profile_all")
    int prof_n = 0, prof_cap = 0;
    hipEvent_t* prof_ev = nullptr;      // 2 per launch
    double* prof_flops = nullptr;
    double* prof_bytes = nullptr;       // algorithmic operand + result bytes of each launch
    float* prof_ms = nullptr;           // filled by pevit_profile_end
    int* prof_shape = nullptr;          // epilogue, M, N, K of each launch
    // A/B-measurement knobs (pevit_tune): per context, so that contexts stay independent of each other
    GemmTune tune;
    hipEvent_t step_gate = nullptr;         // pevit_set_step_gate: the fused step waits for it between the stem and the first block
    const unsigned* ext_poison = nullptr;   // pevit_set_external_poison: a second error word that withholds the optimizer update (the DP exchange's)
    const float* dfeatb_of = nullptr;       // the dfeat buffer whose bf16 copy the head's BatchNorm backward has just left in w_dfeatb (consumed by the next visual backward)
    float* last_loss = nullptr;             // where the loss of the step in flight was written (NaN goes there when its update is withheld)
    // path knobs (pevit_tune), read by plan_step() only
    int gstream16 = 1;        // attention-site adapters, bf16 weights: the residual GRADIENT stream is carried in bf16 only (the copy the dX GEMMs read), LayerNorm backward read-modify-writes it in place: 10 instead of 16 B per element (round 5)
    int dx_stored = 1;        // dX GEMMs hand the LN-input gradient to LayerNorm backward in the activation storage type (bf16)
    int lowrank_combo = 1;    // attention-site adapters: u + dQ + d bias of a layer and the dP of the layer before it as one launch
    int adapter_fused = 1;    // post-MLP adapters: LayerNorm -> down -> activation -> up -> residual (and its backward) as one launch each
    int adapter_tn_fold = 1;  // ... and the two token-contracted weight-gradient products ride in the backward launch (adapter_fused.hip: af_tn_range; > 1: that many workgroups for them)
    int fp8_tail = 1;         // fp8 weights: t = xn P as the bf16 tail of the QKV launch (0: a separate small product, as before round 4)
    int fused_attn_delta = 1; // delta-add + attention forward as one launch where the geometry allows (attn_delta.hip)
    int lowrank_xcd = 1;      // lowrank_grad: XCD-contiguous workgroup order (+0.2 % per step)
};

namespace pevit_host __attribute__((visibility("hidden"))) {

inline bool attention_site(const pevit_ctx* c) {
    return c->d.method == PEVIT_KADAPTATION || c->d.method == PEVIT_LORA;
}
// bytes between the Q panels of two slots of a layer
inline size_t q16_slot_bytes(const pevit_ctx* c) { return align_up((size_t)c->E * 64 * 2, 256); }
inline bool post_mlp(const pevit_ctx* c) { return c->d.method == PEVIT_ADAPTER || c->d.method == PEVIT_COMPACTER; }
// slots of the attention site (rows of wqkv, Q panels, columns of t): those of a multi-slot context of an attention-site method
inline int site_slots(const pevit_ctx* c) { return post_mlp(c) ? 0 : c->slots; }
// bytes between the down (or up) panels of two slots of a layer of a post-MLP slot context
inline size_t pm_slot_bytes(const pevit_ctx* c) { return align_up((size_t)c->E * 64 * c->es, 256); }
// activation of the post-MLP bottleneck as the fused kernels take it: 0 = ReLU (Adapter), 1 = gelu_new (Compacter)
inline int act_kind(const pevit_ctx* c) { return c->d.method == PEVIT_ADAPTER ? 0 : 1; }

template <typename T>
inline T* at(char* base, size_t off) { return reinterpret_cast<T*>(base + off); }
// advance a bf16-declared pointer by `elems` elements of the context's storage type (bf16, or f32 in verification mode)
inline bf16* eadv(const pevit_ctx* c, const bf16* p, size_t elems) {
    return reinterpret_cast<bf16*>(const_cast<char*>(reinterpret_cast<const char*>(p)) + elems * c->es);
}

// ---- ctx.hip ----
StepPlan plan_step(const pevit_ctx* c, int B, bool infer = false);
WsLayout layout_workspace(const pevit_ctx* c, int B, bool infer = false);
int refuse_text(const pevit_ctx* c, const char* who);
int refuse_infer(const pevit_ctx* c, const char* who);
int check_saved(const pevit_ctx* c, Saved want, int B, int layer, const char* who);
int check_ready(pevit_ctx* c, int B, const char* who);

// ---- profile.hip ----
int prof_open(pevit_ctx* c, hipStream_t s, bool is_gemm);
void prof_close(pevit_ctx* c, hipStream_t s, int slot, double flops, double bytes, int s0, int s1, int s2, int s3);
int gemm(pevit_ctx* c, int epi, const GemmParams& p_in, hipStream_t s);

// ---- walk.hip ----
int prep_adapters(pevit_ctx* c, hipStream_t s, int slot = -1, const float* params = nullptr, const float* phm_rule = nullptr);
int attn_core_fwd(pevit_ctx* c, hipStream_t s, int B, const StepPlan& pl, int l, unsigned char* a8, unsigned char* attn8);
int blocks_forward(pevit_ctx* c, hipStream_t s, int B, const StepPlan& pl, bool cls_only, int l_lo = 0, int l_hi = -1);
int attn_core_bwd(pevit_ctx* c, hipStream_t s, int B, const StepPlan& pl, int l, bool cls, AttnGradWalk& w);
int attn_qkv_dx(pevit_ctx* c, hipStream_t s, int B, const StepPlan& pl, int l, float* dx_f32);
int attn_walk_end(pevit_ctx* c, hipStream_t s, int B, AttnGradWalk& w);
int blocks_backward(pevit_ctx* c, hipStream_t s, int B, const StepPlan& pl, bool need_dx0, bool cls_only, int l_hi, int l_lo);
int reduce_adapter_grads(pevit_ctx* c, hipStream_t s, int B, const StepPlan& pl, int l_lo, int l_hi);

// ---- ops.hip, which does not see this header: the process-wide tune of the context-free entry points (pevit_tune with a null
// context sets it) and their stream-K workspace (pevit_streamk_error with a null context reads its error word)
extern GemmTune g_default_tune;
int op_sk_workspace(GemmParams& p);

// CHECK() of a non-GEMM launch, bracketed when "profile_all" is on: kind = PEVIT_PROF_*, bytes = what the launch must move
#define PROF(c, s, kind, rows, bytes, call)                                                  \
    do {                                                                                     \
        const int _slot = prof_open(c, s, false);                                            \
        const int _rc = (call);                                                              \
        prof_close(c, s, _slot, 0.0, (double)(bytes), 100 + (kind), (int)(rows), 0, 0);      \
        if (_rc != 0) return -1;                                                             \
    } while (0)

inline GemmParams gp(const bf16* A, int lda, const bf16* B, int ldb, int Nb, int M, int N, int K) {
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.A = A; p.lda = lda; p.B = B; p.ldb = ldb; p.Nb = Nb; p.M = M; p.N = N; p.K = K;
    return p;
}

// frozen weight operand of layer-l products: bf16, or e4m3 codes + channel scales (ctx->fp8).  `scale_off` = arena offset
// of the per-output-channel scales for the FORWARD products, 0 for the dX products (their scales ride on the A operand).
inline GemmParams gpw(const pevit_ctx* c, const bf16* A, int lda, size_t w_off, int ldb, int Nb, int M, int N, int K, size_t scale_off) {
    GemmParams p = gp(A, lda, at<bf16>(c->arena, w_off), ldb, c->fp8 ? (int)align_up((size_t)Nb, 256) : Nb, M, N, K);
    if (c->fp8) {
        p.b_fp8 = 1;
        p.bscale = scale_off ? at<float>(c->arena, scale_off) : nullptr;
    }
    return p;
}

// operands of the attention core of layer l as its forward left them in the saved slots: q / k / v planes (head layout), attn_out, lse
inline AttnArgs attn_args(const pevit_ctx* c, int B, int l) {
    const LayerSaved& v = c->lay.sav[l];
    const bf16* qkv = at<bf16>(c->ws, v.qkv);
    const size_t plane = (size_t)B * c->N * c->E;
    AttnArgs a;
    a.q = qkv; a.k = eadv(c, qkv, plane); a.v = eadv(c, qkv, 2 * plane);
    a.out = at<bf16>(c->ws, v.attn_out); a.ldo = c->E; a.lse = at<float>(c->ws, v.lse);
    a.B = B; a.H = c->H; a.N = c->N;
    return a;
}

}  // namespace pevit_host
