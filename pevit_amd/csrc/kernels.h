// Internal launcher interface between the C-ABI layer (ctx.hip, profile.hip, walk.hip, step.hip, ops.hip) and the kernel files.
// Convention: a launcher with many operands takes ONE parameter struct (GemmParams, XxxArgs) plus the stream, filled by name at the
// call site.  Every XxxArgs member is default-initialised and an unset member means "absent / off".  The f32 verification twins
// (verify.hip, *_f32) take the SAME struct as their production sibling and reinterpret its bf16-declared members as f32 inside.
#pragma once
#include "common.h"

enum GemmEpilogue {
    EPI_QKV_HEADS = 0,       // +bias, bf16 -> (which, b*H+h, n, d) head layout; cols >= 3E -> f32 t[T][64]
    EPI_BIAS_RESID_F32 = 1,  // out_f32 = acc + bias + resid
    EPI_BIAS_GELU = 2,       // h = acc + bias (bf16, saved) ; g = QuickGELU(h) (bf16)
    EPI_DGELU_BF16 = 3,      // out_bf16 = acc * QuickGELU'(aux)
    EPI_F32 = 4,             // out_f32 = acc
    EPI_BF16 = 5,            // out_bf16 = acc
    EPI_BIAS_BF16 = 6,       // out_bf16 = acc + bias
    EPI_PATCH_EMBED = 7,     // out_f32[b*Ntok+1+g] = acc + pos[1+g]
    EPI_BIAS_RELU_BF16 = 8,  // out_bf16 = relu(acc + bias)
    EPI_BIAS_RESID_KEEP = 9, // out_f32 = acc + bias + resid ; out2_f32 = acc + bias   (post-MLP adapters need h itself)
    EPI_BIAS_GELUNEW = 10,   // a = acc + bias (bf16, saved) ; g = gelu_new(a) (bf16)
    EPI_DRELU_BF16 = 11,     // out_bf16 = acc * (aux > 0)
    EPI_DGELUNEW_BF16 = 12,  // out_bf16 = acc * gelu_new'(aux)
    EPI_BIAS_F32 = 13,       // out_f32 = acc + bias   (MultiheadAttention.forward: out_proj without the block's residual)
    EPI_BIAS_GELU_ONLY = 14, // g = QuickGELU(h) (bf16 or e4m3) of the SAME h = stored(acc + bias) as EPI_BIAS_GELU; h is not written, outb may be null (inference)
};
constexpr int EPI_LAST = EPI_BIAS_GELU_ONLY;

struct GemmParams {
    const bf16* A; int lda;
    const void* B; int ldb; int Nb;   // Nb = readable rows of B (>= N); ldb in elements (bf16, or fp8 codes)
    // fp8 B with a bf16 tail (the QKV product of the attention-site adapters with fp8 frozen weights): output columns >= n_fp8 take
    // their B rows from B2 (bf16, pitch ldb2 elements, Nb2 readable rows) -- the 64 trainable panel rows P_q^T | P_v^T -- inside the
    // same launch (gemm8_kernel only: pevit_gemm_mixed_ok).  n_fp8 must be a multiple of the tile width.  B2 == nullptr: off.
    const bf16* B2; int ldb2, Nb2, n_fp8;
    int b_fp8;                        // B holds e4m3 codes, k-permuted per 128 (fp8_kperm), K % 128 == 0
    int a_fp8;                        // A holds e4m3 codes as well (lda in codes): fp8 x fp8 on the MX matrix instruction (needs b_fp8)
    int out2_fp8;                     // EPI_BIAS_GELU / EPI_BIAS_GELU_ONLY: the activation output (outb2, ldob2 in codes) is written as k-permuted e4m3 codes
    const float* bscale;              // fp8 B: per-output-channel (power-of-two) scale, applied to the accumulator
    const float* oscale;              // EPI_DGELU_BF16 only: per-column factor folded into the bf16 output (or null)
    int M, N, K;
    const float* bias;
    const float* resid; int ldr;
    float* outf; int ldo;
    float* outf2; int ldo2;
    bf16* outb; int ldob;
    bf16* outb2; int ldob2;
    const bf16* aux; int ldaux;
    // head-layout epilogue
    size_t head_stride;   // elements between the q, k and v planes
    int E, H, Ntok;
    int dbg;              // measurement only: bit 0 skips the k-loop, bit 1 the epilogue stores, bit 2 the operand stream, bit 3 ds_read + MFMA
    // stream-K workspace (gemm_streamk.hip gemm_streamk_kernel): one 128x128 f32 slab and one flag per residency slot, or null
    float* sk_slab; unsigned* sk_flag; int sk_slots;
    int sk_share, sk_band;   // set by the launcher: k-iterations per workgroup, m-tiles per band of the tile walk
    int band;                // set by the launcher: m-tiles per band of gemm_device.h tile_origin (0 = TILE_BAND)
    int kz;                  // set by the launcher: K slices per tile across WORKGROUPS (gemm_split.hip gemm_kphase_kernel<..., KZ = true>: 2), else 0
};

// A/B-measurement knobs.  They live in the context (pevit_tune(ctx, ...)); the single-kernel pevit_op_* entry
// points use one process-wide default instance.
struct GemmTune {
    int config = -1;      // -1: per-problem heuristic, >= 0: force a tile configuration (gemm_plan.h kConfigs)
    int persistent = 1;
    int ablate = 0;       // GemmParams::dbg
    int kswitch = 2048;   // K from which the few-tile problems use the 128x128 tile instead of 64x128
    int big = 1;          // allow the 8-wave tiles
    int cfg_longk = 0, cfg_shortk = 1;   // tile configuration of the few-tile problems (N = 768 at M = 6400): K >= kswitch / K < kswitch
    int big_bias = 100;   // the 8-wave tile is taken when its stream cost is below big_bias % of the 128x128 tiling's
    int sk_share = 0, sk_band = 0;   // measurement (gemm_streamk = 2): k-iterations per stream-K workgroup, m-tiles per band
    int ksplit = 1;       // N = E long-K products with ~one 160x128 tile per CU: 8-wave tile, two wave groups on alternate k-tiles
    int ksplit_small = 1;     // ... also as a 96x128 tile where that fills the chip and 160x128 does not (M = 3200)
    int ksplit_stagger = 2;   // ... 1: its two wave groups half an iteration apart (alternate k-tiles); 2: phased kernel (groups split each k-tile, 4 stages)
    int skinny = 1;           // few-row long-K products (M <= skinny_maxm, K >= 64 * skinny_mink): K slices, last arriver sums the slabs (gemm_skinny_kernel)
    int skinny_maxm = 128, skinny_mink = 24, skinny_slices = 0;   // skinny_slices > 0: measurement
    int kz2 = 0;              // ... opt-in (round 5, measured slower): two workgroups per 160x128 tile, half of K each, where those tiles fill at most half the chip (M = 3200, N = 768, long K)
    int kphase_nl = 8;        // ... phased kernel: LDS-DMA pieces per k-tile requested in the LOAD section (the rest between the MFMAs)
    int ksplit_mink = 512;    // ... from this K on
    int band = -1;        // >= 0 forces GemmParams::band of the one-round 8-wave launches (measurement); -1 = XCD-aligned
    int stagger = 1;      // 8-wave tiles (bf16 B): the staggered two-group kernel (gemm8_kernel) instead of gemm_kernel
    int streamk = 1;      // few-tile long-K problems: stream-K decomposition of the 128x128 tiling (needs GemmParams::sk_slab)
};
constexpr int PEVIT_SK_SLAB_FLOATS = 128 * 128;   // one partial tile per residency slot
constexpr int PEVIT_SK_MAX_SLOTS = 1024;
int pevit_gemm_last_path();                        // 1 plain tile, 2 staggered 8-wave, 3 k-split (alternate k-tiles), 4 phased k-split, 5 stream-K, 6 few-row split-K,
                                                   // 7 phased k-split with two K slices per tile
int pevit_gemm_sk_slots();                         // residency slots of the stream-K kernel on this device (2 per CU, multiple of 8)

int pevit_launch_gemm(int epi, const GemmParams& p, const GemmTune& t, hipStream_t stream);
bool pevit_gemm_mixed_ok(const GemmParams& p, const GemmTune& t);   // does pevit_launch_gemm(EPI_QKV_HEADS, p, t) have a kernel that writes the bf16 tail B2?

// ---- norm.hip --------------------------------------------------------------------
// y = LN(x) * gamma + beta over the last dim (eps 1e-5, f32 statistics: model.py:154-160)
struct LnFwdArgs {
    const float* x = nullptr; const float* gamma = nullptr; const float* beta = nullptr;
    int rows = 0, E = 0;
    bf16* y_bf16 = nullptr; float* y_f32 = nullptr; float* mean = nullptr; float* rstd = nullptr;
    size_t xstride = 0;                 // elements between the rows of x (0: E)
    int f32 = 0;
    unsigned char* y_fp8 = nullptr;     // k-permuted e4m3 copy [rows][E]
};
int pevit_launch_ln_fwd(const LnFwdArgs& a, hipStream_t s);
// dx_out = dres + LN-backward(dy)   (gamma/beta frozen: no parameter grads).  dy is f32, or (dy_stored) in the activation
// storage type -- bf16 in production -- when it is the output of a dX GEMM
struct LnBwdArgs {
    const void* dy = nullptr; const float* x = nullptr; const float* mean = nullptr; const float* rstd = nullptr;
    const float* gamma = nullptr; const float* dres = nullptr; float* dx_out = nullptr; bf16* dx_bf16 = nullptr;
    int rows = 0, E = 0;
    size_t xstride = 0;                        // elements between the rows of x and of the gradients (0: E)
    const float* bf16_colscale = nullptr;      // fp8 weights: per-column (power-of-two) factors folded into the bf16 output
    int f32 = 0, dy_stored = 0;
    int res_period = 0;                        // > 0: dres is read on rows that are multiples of it only (zero elsewhere)
    int res16 = 0;                             // dres points at bf16 values (may be dx_bf16 itself: in place); dx_out may then be null
    const float* res_colscale = nullptr;       // res16 + fp8 weights: the power-of-two column scales folded into dres (taken out exactly)
};
int pevit_launch_ln_bwd(const LnBwdArgs& a, hipStream_t s);

// ---- attention.hip / attn_probs.hip ----------------------------------------------
// q,k,v: (B*H, N, 64) bf16 (q pre-scaled by 1/8, deltas already added); out: rows (b*N+n), cols h*64+d
struct AttnArgs {
    const bf16* q = nullptr; const bf16* k = nullptr; const bf16* v = nullptr;
    bf16* out = nullptr; int ldo = 0;       // written by attn_fwd, read by attn_bwd
    float* lse = nullptr;                   // written by attn_fwd (null: not written, the inference form), read by attn_bwd and attn_probs
    int B = 0, H = 0, N = 0;
    unsigned char* out_fp8 = nullptr;       // attn_fwd: + e4m3 copy of out, row pitch ldo codes
    // attn_bwd.  dqkv: row layout [T][ld]: cols [0,E) dq, [E,2E) dk, [2E,3E) dv
    const bf16* dout = nullptr; int lddo = 0;
    bf16* dqkv = nullptr; int ld = 0;
    int dout_cls_only = 0;                  // (N <= 64): dout is zero except on token 0 of every image; the other rows are not read
    // attn_probs: softmax probabilities P = exp(q k^T - lse) of the attention core (q, k as attn_fwd takes them, lse as it wrote
    // it): average = 1 -> probs (B, N, N) f32 = mean over the H heads; 0 -> probs (B, H, N, N) f32
    float* probs = nullptr; int average = 0;
};
int pevit_launch_attn_fwd(const AttnArgs& a, hipStream_t s);
// attn_causal.hip: the text tower's attention (query x sees keys y <= x), 1 <= N <= 128, forward only: reads q, k, v, writes out
int pevit_launch_attn_fwd_causal(const AttnArgs& a, hipStream_t s);
int pevit_launch_attn_bwd(const AttnArgs& a, hipStream_t s);
int pevit_launch_attn_probs(const AttnArgs& a, hipStream_t s);

// ---- attn_delta.hip (attention-site adapters fused with the attention core, N <= 64) --------------
// heads per workgroup of the fused forms for this geometry, or 0 when there is none (the two-kernel path is used)
int pevit_attn_delta_hpw(int B, int H, int N);
// delta_add + attn_fwd in one launch: q, v (head layout) are rewritten with q + delta, v + delta (saved for backward)
struct AttnFwdDeltaArgs {
    bf16* q = nullptr; const bf16* k = nullptr; bf16* v = nullptr;
    const float* t = nullptr; const bf16* q16 = nullptr; const float* bias = nullptr; float ascale = 0.f;
    bf16* out = nullptr; int ldo = 0; float* lse = nullptr;
    int B = 0, H = 0, N = 0;
    int nosave = 0;     // inference: q' / v' stay in LDS and lse is not written (q, v are only read; lse may be null); same `out`
};
int pevit_launch_attn_fwd_delta(const AttnFwdDeltaArgs& a, hipStream_t s);

// ---- segmented forms of the attention site (pevit_predict_segments): the batch is split into contiguous segments of images, and
// the raw reshape of the delta works INSIDE each segment (local reference row rr: token rr / count of image first + rr % count), with
// that segment's Q panel, bias and 64 columns of t.  Inference only: q and v are only read by the fused form.
constexpr int PEVIT_MAX_SEGMENTS = 16;
struct AttnSegment {
    int first = 0, count = 0;           // images [first, first + count) of the batch
    int tcol = 0;                       // first of this segment's 64 columns of t
    const bf16* q16 = nullptr;          // its [E][64] bf16 panel of Q
    const float* bias = nullptr;        // its delta bias [E], or null
};
struct AttnSiteSegArgs {
    bf16* q = nullptr; const bf16* k = nullptr; bf16* v = nullptr;     // head layout, all B images
    const float* t = nullptr; int tpitch = 64;                         // [B*N][tpitch] f32
    float ascale = 0.f;
    bf16* out = nullptr; int ldo = 0;                                  // (the fused form only)
    int B = 0, H = 0, N = 0;
    int nseg = 0; AttnSegment seg[PEVIT_MAX_SEGMENTS];
};
// the kernels' view, passed by value: wg0[s] = first workgroup of segment s (a run of heads, or a group of reference rows, never
// crosses a segment).  Entries behind nseg are zero.  NoSegments is the empty table of the unsegmented instances: every use of the
// table sits under `if constexpr (SEG::on)`, so those instances keep their code.
struct NoSegments { static constexpr bool on = false; };
struct SegTable {
    static constexpr bool on = true;
    int nseg, tpitch;
    int first[PEVIT_MAX_SEGMENTS], count[PEVIT_MAX_SEGMENTS], tcol[PEVIT_MAX_SEGMENTS], wg0[PEVIT_MAX_SEGMENTS];
    const bf16* q16[PEVIT_MAX_SEGMENTS]; const float* bias[PEVIT_MAX_SEGMENTS];
};
// the host checks both launchers share (segments tile [0, B), t columns inside the pitch); fills everything of `tab` but wg0
int pevit_seg_table(const AttnSiteSegArgs& a, const char* who, SegTable& tab);
// q / v of every segment rewritten in place with q + delta, v + delta (bf16 storage); the unchanged attn_fwd follows
int pevit_launch_delta_add_seg(const AttnSiteSegArgs& a, hipStream_t s);
// delta + attention in one launch, where pevit_attn_delta_hpw allows: one workgroup per run of heads INSIDE a segment
int pevit_launch_attn_fwd_delta_seg(const AttnSiteSegArgs& a, hipStream_t s);

void pevit_attn_delta_set_timeline(void* buf);     // measurement only: 8 s_memtime stamps per workgroup of the next fused launches (null = off)

// ---- lowrank.hip -----------------------------------------------------------------
struct AdapterPanels {      // per layer, rewritten every step from the f32 master parameters
    bf16* w_aug_rows;       // &Wqkv_aug[3E][0]  : 64 rows x E  (P_q^T | P_v^T)
    int ldw;
    bf16* wT_aug_cols;      // &WqkvT_aug[0][3E] : E rows, 64 cols (ascale*P_q | ascale*P_v)
    int ldwT;
    float* q32;             // [E][64] f32 : Q_q | Q_v
    bf16* qT;               // [64][E] bf16: Q_q^T ; Q_v^T
    bf16* q16;              // [E][64] bf16: Q_q | Q_v (operand of the forward delta; bf16 storage only)
};
struct LayerStrides { size_t arena_bytes; size_t param_floats; };   // per-layer pointer advance
// KAdaptation: P[:,j] = s_j (x) l_j , Q[:,j] = t_j (x) r_j   (model.py:567-580); all layers
struct PrepKadaptArgs {
    const float* rule1_l = nullptr; const float* rule1_r = nullptr; const float* rule2_l = nullptr; const float* rule2_r = nullptr;
    const float* q_left = nullptr; const float* q_right = nullptr;
    AdapterPanels pan{}; int E = 0; float ascale = 0.f; int layers = 0; LayerStrides st{}; int f32 = 0;
};
int pevit_launch_prep_kadapt(const PrepKadaptArgs& a, hipStream_t s);
// LoRA: P_q = A1q^T, Q_q = A2q (rank r zero-padded to 32)   (lora_model.py:490-514); all layers
struct PrepLoraArgs {
    const float* a1q = nullptr; const float* a2q = nullptr; const float* a1v = nullptr; const float* a2v = nullptr; int r = 0;
    AdapterPanels pan{}; int E = 0; float ascale = 0.f; int layers = 0; LayerStrides st{}; int f32 = 0;
};
int pevit_launch_prep_lora(const PrepLoraArgs& a, hipStream_t s);
// q_buf_flat[rr*E+e] += ascale * t[row(rr)][0:32] . Q_q[e] + bias[e]   (and v with cols 32:64)
// rr is the reference's (n*B+b) row index of the raw reshape (model.py:796-799); row(rr)=b*N+n.
struct DeltaAddArgs {
    bf16* qbuf = nullptr; bf16* vbuf = nullptr; const float* t = nullptr;
    const float* q32 = nullptr;     // the f32 panel [E][64] of Q (f32 verification mode)
    const bf16* q16 = nullptr;      // the bf16 panel [E][64] of Q (production operand)
    const float* bias = nullptr; float ascale = 0.f;
    int B = 0, N = 0, E = 0, f32 = 0;
};
int pevit_launch_delta_add(const DeltaAddArgs& a, hipStream_t s);
// The backward kernels of the attention-site adapters share their operands:
//   lowrank_u:     u[row(rr)][0:32] = dDelta_q[rr] . Q_q ; [32:64] = dDelta_v[rr] . Q_v ; written f32 (u32) and bf16 into
//                  u_bf16_cols = dqkv[:, 3E:3E+64]
//   lowrank_grad:  partial[chunk][4][E][32]: dP_q, dP_v (= xn^T u), dQ_q, dQ_v (= dDelta^T t_ref); dbias_partial[chunk][E]
//   lowrank_combo: u + dQ / d bias of this layer and the deferred dP of the previously processed layer in ONE launch
//                  (lowrank_combo_kernel)
struct LowrankArgs {
    const bf16* dqkv = nullptr; int ld = 0;
    const bf16* qT = nullptr;               // [64][E] panel of Q^T (production)
    const float* q32 = nullptr;             // [E][64] f32 panel of Q (lowrank_u_f32 only)
    float* u32 = nullptr; bf16* u_bf16_cols = nullptr;
    const bf16* xn = nullptr; int ldx = 0;  // lowrank_grad: LayerNorm output of this layer ; ldx also the pitch of xn_prev
    const float* t = nullptr;
    float* partial = nullptr; float* dbias_partial = nullptr;
    int chunks = 0;                         // lowrank_grad: pevit_lowrank_chunks(B * N)
    int B = 0, H = 0, N = 0, E = 0;
    int xcd_order = 1;                      // lowrank_grad: XCD-contiguous workgroup order (measurement knob; on unless cleared)
    // lowrank_combo.  this_layer = 0: only the deferred dP of the previous layer (end of the layer loop); prev = 0: no deferred work
    int this_layer = 0, prev = 0;
    const bf16* xn_prev = nullptr; const float* u32_prev = nullptr; float* partial_prev = nullptr;
};
int pevit_launch_lowrank_u(const LowrankArgs& a, hipStream_t s);
int pevit_launch_lowrank_grad(const LowrankArgs& a, hipStream_t s);
int pevit_lowrank_chunks(int T);
int pevit_launch_lowrank_combo(const LowrankArgs& a, hipStream_t s);
// what the two gradient launchers launch for B * N rows on the current device: es 64-column slabs per gradient workgroup (0: none
// for this width), nu u blocks, n12 dQ blocks, n0 dP blocks, chunks of 256 rows.  combo = 0: lowrank_grad (this_layer, prev ignored)
struct LowrankPlan { int es = 0, nu = 0, n12 = 0, n0 = 0, chunks = 0; };
LowrankPlan pevit_lowrank_plan(int B, int N, int E, int combo, int this_layer, int prev);
// reduce the per-chunk partials of all layers and apply the chain rule onto the reference's
// parameter tensors (flat gradient buffer, accumulating)
struct ChainKadaptArgs {
    const float* partial = nullptr; size_t partial_layer = 0; const float* dbias_partial = nullptr; size_t dbias_layer = 0;
    int chunks = 0; float ascale = 0.f; int layers = 0;
    float* G = nullptr; float* rule_scratch = nullptr; const float* params = nullptr; float* grads = nullptr;
    size_t p_layer0 = 0, p_layer_stride = 0; int E = 0;
};
int pevit_launch_chain_kadapt(const ChainKadaptArgs& a, hipStream_t s);
int pevit_launch_rule_sum(const float* rule_scratch, float* grads, int l_lo, int l_hi, hipStream_t s);
struct ChainLoraArgs {
    const float* partial = nullptr; size_t partial_layer = 0; int chunks = 0; float ascale = 0.f; int r = 0, layers = 0;
    float* G = nullptr; float* grads = nullptr; size_t p_layer0 = 0, p_layer_stride = 0; int E = 0;
};
int pevit_launch_chain_lora(const ChainLoraArgs& a, hipStream_t s);

// ---- misc.hip --------------------------------------------------------------------
int pevit_launch_cast_bf16(const float* src, bf16* dst, size_t n, float scale, hipStream_t s, int f32 = 0);
// dst[c][r] = scale(r) * src[r][c]  (bf16 out), used once at load for the backward weights
int pevit_launch_transpose_bf16(const float* src, int rows, int cols, bf16* dst, int ldd,
                                int scaled_rows, float scale, hipStream_t s, int f32 = 0);
int pevit_launch_permute_rows(const float* src, float* dst, int N, int B, int E, int to_internal,
                              hipStream_t s);
int pevit_launch_scale_f32(float* p, size_t n, float scale, hipStream_t s);
int pevit_launch_zero(void* ptr, size_t bytes, hipStream_t s);      // the step's memsets as a kernel (capturable in order into a HIP graph)
struct SgdArgs {
    float* p = nullptr; const float* g = nullptr; float* mom = nullptr; const unsigned char* has_grad = nullptr; size_t n = 0;
    float lr = 0.f, momentum = 0.f, wd = 0.f; int first_step = 0; float grad_scale = 0.f;
    const unsigned* poison = nullptr;     // device word: non-zero = skip the update (stream-K hand-off error)
    unsigned* skipped = nullptr;          // device counter of the updates skipped that way
    const unsigned* poison2 = nullptr;    // a second such word (the data-parallel exchange's)
    float* loss_slot = nullptr;           // where the step's loss sits: NaN goes there when the update is withheld
};
int pevit_launch_sgd(const SgdArgs& a, hipStream_t s);

// ---- optim.hip (Adam, AdamW and per-group SGD over the flat parameter buffer) ------------------------
enum OptimKind { OPTIM_SGD = 0, OPTIM_ADAM = 1, OPTIM_ADAMW = 2 };      // == enum pevit_optim_kind (include/pevit_hip.h)
constexpr int OPTIM_MAX_GROUPS = 8;
// one parameter group as the kernel reads it: every scalar derived from the caller's double-precision hyper-parameters is
// rounded to f32 once, on the host (torch hands its Python scalars to the f32 kernels the same way)
struct OptimGroup {
    float lr = 0.f, wd = 0.f, momentum = 0.f;                 // SGD
    float w1 = 0.f, beta2 = 0.f, w2 = 0.f, eps = 0.f;         // Adam kinds: 1 - beta1, beta2, 1 - beta2, eps
    float step_size = 0.f, sqrt_bc2 = 1.f;                    // lr / (1 - beta1^t), sqrt(1 - beta2^t)
    float decay = 1.f;                                        // AdamW: 1 - lr * wd
    int nesterov = 0;
};
// passed to the kernel BY VALUE (the groups included): no host-to-device copy on the step
struct OptimArgs {
    float* p = nullptr; const float* g = nullptr; float* exp_avg = nullptr; float* exp_avg_sq = nullptr;   // exp_avg: the momentum buffer
    const unsigned char* group_of = nullptr;   // per element: index into groups; 255 = the parameter's .grad is None (skipped)
    size_t n = 0;
    int kind = OPTIM_SGD, n_groups = 0, first_step = 0; float grad_scale = 0.f;
    const unsigned* poison = nullptr;     // as in SgdArgs: error words that withhold the update,
    unsigned* skipped = nullptr;          // the counter of withheld updates
    const unsigned* poison2 = nullptr;
    float* loss_slot = nullptr;           // and where NaN goes when it is withheld
    OptimGroup groups[OPTIM_MAX_GROUPS];
};
int pevit_launch_optim(const OptimArgs& a, hipStream_t s);

// ---- clip.hip (gradient-norm clipping over the flat gradient buffer: clip_grad_norm_, norm_type 2) ----
constexpr int CLIP_CHUNK = 8192;          // elements of the slice one workgroup of grad_sumsq_kernel / grad_scale_kernel owns
struct ClipArgs {
    float* g = nullptr;                   // the flat buffer, 16-byte aligned; scaled in place
    const unsigned char* mask = nullptr;  // optional, 4-byte aligned: elements whose byte is 0 are neither counted nor scaled
    size_t n = 0;
    float max_norm = 0.f, grad_scale = 1.f;      // grad_scale multiplies the NORM only (1 / world under data parallelism)
    float* scratch = nullptr;             // pevit_clip_scratch_floats(n) words: {total, coef, ticket, -, one partial per workgroup}
};
size_t pevit_clip_blocks(size_t n);       // workgroups (= partials) of both launches
int pevit_clip_check(float max_norm, float grad_scale, const char* who);     // both finite and > 0, or -1 with the error text set
int pevit_launch_grad_sumsq(const ClipArgs& a, hipStream_t s);               // scratch[0] = total, scratch[1] = coef
int pevit_launch_grad_scale(const ClipArgs& a, hipStream_t s);               // g *= scratch[1]

int pevit_launch_occupy(int blocks, int lds_bytes, double micros, hipStream_t s);   // measurement only (pevit_debug_occupy)

// ---- fp8.hip (e4m3 codes + power-of-two channel scales of the frozen weights) -----------------
int pevit_launch_quant_rows_fp8(const float* W, int rows, int cols, unsigned char* out, int ldo, float* scale, int scaled_rows,
                                float pre, hipStream_t s);
int pevit_launch_quant_transpose_fp8(const float* W, int rows, int cols, const float* scale, unsigned char* outT, int ldo,
                                     int scaled_rows, float pre, hipStream_t s);
int pevit_launch_cast_bf16_cols(const float* src, bf16* dst, size_t rows, int cols, const float* colscale, hipStream_t s);
int pevit_launch_cast_fp8(const float* src, unsigned char* dst, size_t rows, int cols, hipStream_t s);
int pevit_launch_dequant_rows_fp8(const unsigned char* codes, int ldc, const float* scale, int rows, int cols, float* out,
                                  hipStream_t s);

// ---- adapter.hip (post-MLP bottleneck adapters: Adapter, Compacter) -------------------------------
struct BottleneckPanels { bf16* wd; bf16* wdT; bf16* wu; bf16* wuT; };   // [64][E], [E][64], [E][64], [64][E]
int pevit_tn_chunks(int T);
int pevit_lna_blocks(int rows);
int pevit_launch_prep_adapter(const float* w_down, const float* w_up, BottleneckPanels pan, int E, int layers, LayerStrides st,
                              hipStream_t s, int f32 = 0);
struct PrepCompacterArgs {
    const float* rule = nullptr; const float* dWl = nullptr; const float* dWr = nullptr; const float* uWl = nullptr;
    const float* uWr = nullptr;
    BottleneckPanels pan{}; int E = 0, layers = 0; LayerStrides st{}; int f32 = 0;
};
int pevit_launch_prep_compacter(const PrepCompacterArgs& a, hipStream_t s);
// G[e][j] = sum_r X[r][e] Y[r][j] (per-chunk partials [chunk][E][64]); optional column sums of X / Y
struct TnGemm64Args {
    const bf16* X = nullptr; int ldx = 0; const bf16* Y = nullptr; int ldy = 0;
    float* partial = nullptr; float* csx = nullptr; float* csy = nullptr; int T = 0, E = 0;
};
int pevit_launch_tn_gemm64(const TnGemm64Args& a, hipStream_t s);
struct LnBwdAffineArgs {
    const float* dy = nullptr; const float* x = nullptr; const float* mean = nullptr; const float* rstd = nullptr;
    const float* gamma = nullptr; const float* dres = nullptr; float* dx = nullptr; bf16* dx_bf16 = nullptr;
    float* partial = nullptr; int rows = 0, E = 0, f32 = 0;
};
int pevit_launch_ln_bwd_affine(const LnBwdAffineArgs& a, hipStream_t s);
// ---- adapter_fused.hip: the post-MLP adapter as one launch per direction (bf16 storage, E a multiple of 256) ----
bool pevit_adapter_fused_ok(int E);
int pevit_num_cus();                 // compute units of the current device (cached)
int pevit_adapter_blocks(int T);     // workgroups (= blocks of LayerNorm-affine partials) of the fused backward
// act_kind 0 = ReLU (Adapter), 1 = gelu_new (Compacter).  hraw = c_proj accumulators WITHOUT their bias (f32), bpr = that bias.
struct AdapterFwdArgs {
    int act_kind = 0;
    const float* hraw = nullptr; const float* bpr = nullptr; const float* x_mid = nullptr; const float* gamma = nullptr;
    const float* beta = nullptr; const bf16* wd = nullptr; const float* b_down = nullptr; const bf16* wu = nullptr;
    const float* b_up = nullptr;
    bf16* z = nullptr; float* mean_a = nullptr; float* rstd_a = nullptr; bf16* act = nullptr; bf16* apre = nullptr;
    float* x_out = nullptr; int T = 0, E = 0;
};
int pevit_launch_adapter_fwd(const AdapterFwdArgs& a, hipStream_t s);
// The segmented inference form (pevit_predict_segments on a post-MLP slot context): rows [first, end) of hraw / x_mid / x_out belong
// to a segment with its own LayerNorm affine, panels and biases.  A workgroup never crosses a segment end, and nothing that only a
// backward reads is stored.  x_out of a segment = pevit_launch_adapter_fwd on that segment's rows alone, bit for bit.
struct AdapterSegment {
    int first = 0, end = 0;             // rows [first, end) of the [T][E] buffers
    const float* gamma = nullptr; const float* beta = nullptr; const bf16* wd = nullptr; const float* b_down = nullptr;
    const bf16* wu = nullptr; const float* b_up = nullptr;
};
struct AdapterFwdSegArgs {
    int act_kind = 0;
    const float* hraw = nullptr; const float* bpr = nullptr; const float* x_mid = nullptr; float* x_out = nullptr; int E = 0;
    int nseg = 0; AdapterSegment seg[PEVIT_MAX_SEGMENTS];
};
int pevit_launch_adapter_fwd_seg(const AdapterFwdSegArgs& a, hipStream_t s);
// saved = act (ReLU) / apre (gelu_new); partial: [pevit_lna_blocks(T)][3][E] like ln_bwd_affine
struct AdapterBwdArgs {
    int act_kind = 0;
    const bf16* dyb = nullptr;
    const float* dres = nullptr;        // null: the bf16 gradient stream -- dx_out is read from dyb wherever the f32 copy was
    const bf16* wuT = nullptr; const bf16* saved = nullptr; const bf16* wdT = nullptr;
    const float* hraw = nullptr; const float* bpr = nullptr; const float* mean_a = nullptr; const float* rstd_a = nullptr;
    const float* gamma = nullptr;
    bf16* dpre = nullptr; bf16* dh_bf16 = nullptr; float* partial = nullptr; int T = 0, E = 0;
    // tn_*: the contraction range of the launch (adapter_fused.hip af_tn_range); tn_x1 / tn_x2 unset leave a product out.
    //   product 1: tn_partial1[chunk][E][64] = sum over the chunk's rows of x1[r][e] y1[r][j]   (x1: [T][E] bf16, y1: [T][64] bf16)
    //   product 2: the same for x2, y2 -> tn_partial2, and tn_csy2[chunk][64] = column sums of y2
    const bf16* tn_x1 = nullptr; const bf16* tn_y1 = nullptr; float* tn_partial1 = nullptr;
    const bf16* tn_x2 = nullptr; const bf16* tn_y2 = nullptr; float* tn_partial2 = nullptr; float* tn_csy2 = nullptr;
    int tn_blocks = 0;                  // workgroups of the contraction range, 0 = one per unit pair
};
int pevit_launch_adapter_bwd(const AdapterBwdArgs& a, hipStream_t s);
int pevit_launch_colsum_reduce(const float* partial, int chunks, int n, float* out, int layers, size_t partial_layer,
                               size_t out_layer, hipStream_t s);
struct ColsumReduce3Args {
    const float* partial = nullptr; int chunks = 0, n = 0; float* o0 = nullptr; float* o1 = nullptr; float* o2 = nullptr;
    int layers = 0; size_t partial_layer = 0, out_layer = 0;
};
int pevit_launch_colsum_reduce3(const ColsumReduce3Args& a, hipStream_t s);
int pevit_launch_chain_adapter(const float* Gd, const float* Gu, float* g_down, float* g_up, int E, int layers, size_t g_layer,
                               size_t param_layer, hipStream_t s);
struct ChainCompacterArgs {
    const float* Gd = nullptr; const float* Gu = nullptr; const float* rule = nullptr; const float* params = nullptr;
    float* grads = nullptr; int E = 0, layers = 0; size_t g_layer = 0, param_layer = 0;
    size_t off_dWl = 0, off_dWr = 0, off_uWl = 0, off_uWr = 0;
};
int pevit_launch_chain_compacter(const ChainCompacterArgs& a, hipStream_t s);

// ---- verify.hip (f32-class verification mode: plain f32 kernels for the matrix-core contractions) -----------------
// Each twin takes its production sibling's struct; the members declared bf16 (and lowrank_grad's xn) hold f32 there.
int pevit_launch_gemm_f32(int epi, const GemmParams& p, hipStream_t s);      // A, B and the bf16-declared buffers hold f32
int pevit_launch_attn_fwd_f32(const AttnArgs& a, hipStream_t s);             // (out_fp8 is not written)
int pevit_launch_attn_fwd_causal_f32(const AttnArgs& a, hipStream_t s);      // (no lse)
int pevit_launch_attn_bwd_f32(const AttnArgs& a, hipStream_t s);             // (every row of dout is read: dout_cls_only has no effect)
int pevit_launch_attn_probs_f32(const AttnArgs& a, hipStream_t s);
int pevit_launch_lowrank_u_f32(const LowrankArgs& a, hipStream_t s);         // reads the f32 panel q32, not qT
// G[e][j] = sum_r X[r][e] Y[r][j], partial / column-sum layout of tn_gemm64 (adapter.hip)
int pevit_launch_tn_gemm64_f32(const TnGemm64Args& a, hipStream_t s);
int pevit_launch_lowrank_grad_f32(const LowrankArgs& a, hipStream_t s);      // (no workgroup-order knob)

// ---- text.hip (CLIP text tower: token-embedding stem and the end-of-text gather) ---------------------------------
// x[s*N + n][:] = table[clamp(tokens[s][n], 0, V - 1)][:] + pos[n][:]   (f32; model.py:1154)
struct TextEmbedArgs {
    const int64_t* tokens = nullptr; const float* table = nullptr; const float* pos = nullptr; float* x = nullptr;
    int S = 0, N = 0, E = 0, V = 0;
};
int pevit_launch_text_embed(const TextEmbedArgs& a, hipStream_t s);
// rows_out[s][:] = x[s*N + argmax_n tokens[s][n]][:], the first maximum (model.py:1166); ln_final runs on the compact rows
int pevit_launch_text_eot_gather(const int64_t* tokens, const float* x, float* rows_out, int S, int N, int E, hipStream_t s);

// ---- stem_head.hip -----------------------------------------------------------------
int pevit_launch_im2col(const float* img, bf16* out, int B, int R, int P, int Kp, hipStream_t s, int f32 = 0);
// uint8 pixels with ToTensor + Normalize folded in: x = (u8 / 255 - mean[c]) / std[c] (feature.py:537-542)
struct Im2colU8Args {
    const unsigned char* img = nullptr; const float* mean3 = nullptr; const float* std3 = nullptr; bf16* out = nullptr;
    int B = 0, R = 0, P = 0, Kp = 0, f32 = 0;
};
int pevit_launch_im2col_u8(const Im2colU8Args& a, hipStream_t s);
int pevit_launch_conv_weight(const float* w, bf16* out, int E, int K, int Kp, hipStream_t s, int f32 = 0);
int pevit_launch_cls_row(const float* cls, const float* pos, float* x, int B, int N, int E, hipStream_t s);
// labels (B) int64 -> cross-entropy; targets (B x C) f32 -> BCE with logits; both null -> forward only
struct HeadArgs {
    const float* feat = nullptr; const int64_t* labels = nullptr; const float* targets = nullptr;
    const float* W = nullptr; const float* bias = nullptr; float* gW = nullptr; float* gb = nullptr;
    float* running_mean = nullptr; float* running_var = nullptr; int training = 0;
    float* ybn = nullptr; float* rstd = nullptr; float* logits = nullptr; float* dlogits = nullptr; float* dybn = nullptr;
    float* loss = nullptr; float* dfeat = nullptr; int B = 0, D = 0, Cc = 0;
    bf16* dfeat_bf16 = nullptr;     // bf16 copy of dfeat written by the BatchNorm backward (no cast launch)
};
int pevit_launch_head(const HeadArgs& a, hipStream_t s);

// ---- zeroshot.hip (the CLIP zero-shot head: cosine logits and their softmax in one launch, exact f32) ------------
// logits[b][c] = scale / max(||feat_b||, 1e-12) * <feat_b, text_c> ; probs[b][:] = softmax(logits[b][:])
// feat [B][D], text [C][D] (class-major unit rows), outputs [B][C], all f32; either output may be null, not both.
// 1 <= C <= 1024, D a multiple of 8 up to 1024, B >= 1, feat and text 16-byte aligned: pevit_zeroshot_check refuses the rest.
struct ZeroshotArgs {
    const float* feat = nullptr; const float* text = nullptr; float* probs = nullptr; float* logits = nullptr;
    float scale = 100.f;
    int B = 0, D = 0, C = 0;
};
int pevit_zeroshot_check(const ZeroshotArgs& a);      // 0, or -1 with the error text set; launches nothing
int pevit_launch_zeroshot_head(const ZeroshotArgs& a, hipStream_t s);

// ---- probe.hip (the linear probe's head on cached feature rows: a two-launch training step and a one-launch predict) ----
// feat [rows][D] f32 (16-byte aligned); index [B] int64 rows of feat, or null: rows row0 .. row0 + B - 1; labels [rows] int64
// (cross-entropy) or targets [rows][C] f32 (BCE with logits), indexed like feat.  pW / pB, gW / gB, mW / mB: the head's weight
// [C][D] and bias [C] in the parameter, gradient and momentum buffers.  xhat [B][D], dlogits [B][C], rowloss [B + 1] (the row losses, then the count of non-ignored rows): scratch that
// launch 1 hands to launch 2.  D a multiple of 16 up to 1024, C <= 1024: pevit_probe_check refuses the rest.
struct ProbeArgs {
    const float* feat = nullptr; const int64_t* index = nullptr; const int64_t* labels = nullptr; const float* targets = nullptr;
    const float* W = nullptr; const float* bias = nullptr;
    float* pW = nullptr; float* pB = nullptr; float* gW = nullptr; float* gB = nullptr; float* mW = nullptr; float* mB = nullptr;
    float* running_mean = nullptr; float* running_var = nullptr;
    float* xhat = nullptr; float* dlogits = nullptr; float* rowloss = nullptr; float* logits = nullptr; float* loss = nullptr;
    long rows = 0, row0 = 0;
    int B = 0, D = 0, C = 0, training = 0, update = 0, flags = 0;      // flags: bit 0 = first step, bit 1 = Nesterov (pevit_sgd_step)
    float scale = 1.f, lr = 0.f, momentum = 0.f, wd = 0.f;
};
int pevit_probe_check(int D, int C, const char* who);      // 0, or -1 with the error text set; launches nothing
int pevit_launch_probe_step(const ProbeArgs& a, hipStream_t s);
int pevit_launch_probe_predict(const ProbeArgs& a, hipStream_t s);

// ---- resize.hip (Pillow's 8-bit bicubic resize + centre crop of uint8 planes, bit for bit; tables from resize_plan.hip) ----
// src [planes][src_h][src_w] -> dst [planes][out_h][out_w], both uint8 and dense.  kh [out_w][ksize_h] / kv [out_h][ksize_v]: int32
// taps with 22 fractional bits; bh [out_w][2] / bv [out_h][2]: (first source sample, taps) per output column / row, all in device
// memory.  The crop is the choice of table rows.  1 <= src_h, src_w <= 4096, out_h, out_w <= 256, ksize_h, ksize_v <= 33:
// pevit_resize_check refuses the rest.  Table contents are clamped on the device: a wrong table gives wrong pixels, never an
// access outside src, dst or the tables.
struct ResizeArgs {
    const uint8_t* src = nullptr; uint8_t* dst = nullptr;
    const int32_t* kh = nullptr; const int32_t* bh = nullptr; const int32_t* kv = nullptr; const int32_t* bv = nullptr;
    int planes = 0, src_h = 0, src_w = 0, out_h = 0, out_w = 0, ksize_h = 0, ksize_v = 0;
    int lds_rows = 0, ldw = 0;       // set by the launcher: rows and row pitch of the intermediate in LDS
};
int pevit_resize_check(const ResizeArgs& a);          // 0, or -1 with the error text set; launches nothing
int pevit_launch_resize_u8(ResizeArgs a, hipStream_t s);

// ---- resize_ragged.hip (the same resize with the geometry per image: a pool of (3, h_i, w_i) blocks -> dense [batch][3][out][out]) ----
// pool: the images' bytes, one block after the other; desc [n_images]: per image of the set its block's byte offset, h, w and, per
// axis, the element offsets of its table rows in k_pool (int32 taps, out x ksize) and b_pool (int32 (first, taps), out x 2) and its
// ksize (pevit_resize_ragged_desc, include/pevit_hip.h).  Output image b is image index[b] (b itself when index is null).
// max_ksize_v: the largest ksize_v of desc, which sizes the LDS.  All pointers are device memory.  Every index is clamped on the device.
struct pevit_resize_ragged_desc;
struct ResizeRaggedArgs {
    const uint8_t* pool = nullptr; const pevit_resize_ragged_desc* desc = nullptr;
    const int32_t* k_pool = nullptr; const int32_t* b_pool = nullptr; const int64_t* index = nullptr; uint8_t* dst = nullptr;
    long long pool_bytes = 0, k_len = 0, b_len = 0;
    int n_images = 0, batch = 0, out = 0, max_ksize_v = 0;
    int lds_rows = 0, ldw = 0;       // set by the launcher: rows and row pitch of the intermediate in LDS
};
int pevit_launch_resize_ragged_u8(ResizeRaggedArgs a, hipStream_t s);     // 0, or -1 with the error text set before any launch
