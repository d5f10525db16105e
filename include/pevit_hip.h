/* pevit_hip.h -- C ABI of the MI355X (gfx950) engine for parameter-efficient fine-tuning of
 * CLIP vision transformers.
 *
 * The reference (eric-ai-lab/PEViT) has no FFI/plugin layer: its hot path sits behind plain
 * PyTorch module methods.  This header declares the drop-in boundary for that path; every
 * entry point names the reference interface it replaces (paths relative to
 * vision_benchmark/evaluation/ of the reference):
 *
 *   pevit_transformer_forward / _backward   Transformer.forward            model.py:1013-1014
 *                                           = 12 x ResidualAttentionBlock.forward  model.py:972-975
 *                                           incl. MultiheadAttention.multi_head_attention_forward
 *                                           (model.py:612-834) and adapter_forward (model.py:563-584;
 *                                           lora_model.py:490-514), and their autograd backward
 *   pevit_attention_forward / _backward     MultiheadAttention.forward(x, x, x, need_weights, attn_mask=None,
 *                                           average_attn_weights)  model.py:837-944 (-> 612-834) of one block
 *                                           (resblocks[i].attn), incl. the head-averaged / per-head weights
 *   pevit_visual_forward / _backward        VisionTransformer.forward      model.py:1034-1051
 *                                           (= CLIP.encode_image, model.py:1151-1152)
 *   pevit_predict                           Classifier.forward in eval mode (validate's model(images)): images -> logits
 *                                           kadaptation_clip.py:176-185, 395
 *   pevit_head_forward_backward             Classifier.forward tail + CrossEntropyLoss
 *                                           kadaptation_clip.py:128-132,176-185,276,351-352
 *   pevit_sgd_step                          optimizer.step()               kadaptation_clip.py:353,
 *                                           optim/build.py:120-127
 *   pevit_optim_step                        optimizer.step() of Adam / AdamW / SGD with several groups
 *                                           optim/build.py:107-170
 *   pevit_load_block / pevit_load_stem      build_model's load_state_dict  model.py:1247-1250
 *
 * Conventions: extern "C"; every function returns 0 on success and a negative value on error
 * (pevit_last_error() gives the message); nothing throws; no device-memory allocation by any context entry point
 * (profiling creates its events in pevit_profile_begin; the CONTEXT-FREE test entry point pevit_op_gemm allocates a stream-K
 * workspace of its own on first use, once per process).  One process drives one device: the kernel attributes and the CU count are cached
 * per process -- all device memory (weight arena, workspace, parameter and gradient
 * buffers) is owned by the caller and only borrowed; all work is enqueued asynchronously on
 * the caller's hipStream_t (passed as void*); contexts are independent of each other (no
 * mutable process-wide state on the hot path; tuning knobs live in the context) but one context
 * is not thread-safe, matching the reference's single-threaded caller.
 *
 * Row order: the reference keeps activations sequence-first, (N, B, E).  Entry points with
 * "_nbe" arguments take and return exactly that layout; internally rows are batch-major.
 */
#ifndef PEVIT_HIP_H
#define PEVIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pevit_ctx pevit_ctx;

enum pevit_method {
    PEVIT_KADAPTATION = 0, /* model.py          : Kronecker rank-32 delta on q and v + shared bias b */
    PEVIT_LORA = 1,        /* lora_model.py     : low-rank A.B on q and v, scale alpha/r            */
    PEVIT_ADAPTER = 2,     /* adapter_model.py  : bottleneck adapter after the MLP                  */
    PEVIT_COMPACTER = 3,   /* compacter_model.py: PHM (n=4) bottleneck adapter after the MLP        */
    PEVIT_NONE = 4         /* frozen tower, no adapter (linear probe)                               */
};

enum pevit_weight_format {
    PEVIT_W_BF16 = 0,     /* frozen block weights rounded to bf16 (reference: fp32 parameters, model.py:1247-1250)    */
    PEVIT_W_FP8_E4M3 = 1, /* OCP e4m3 codes + one power-of-two f32 scale per output channel, packed by
                             pevit_load_block; activations stay bf16, accumulation f32 (BASELINE config 5).  Bit-identical
                             to PEVIT_W_BF16 run on the de-quantised weights.  KAdaptation, LoRA and the frozen tower.  */
    PEVIT_W_FP8_ACT = 3,  /* opt-in, NOT bit-compatible with the bf16 path: PEVIT_W_FP8_E4M3 weights, and in the FORWARD pass the
                             A operands of the four frozen products of a block (LayerNorm outputs, attention output, gelu(h))
                             are e4m3 codes too (unscaled: activations are O(1); saturating at +-448), written by their
                             producers, so that these products run fp8 x fp8 on CDNA4's MX-scaled matrix instruction
                             (v_mfma_scale_f32_32x32x64_f8f6f4 with unit block scales: twice the bf16 MFMA rate, half the
                             operand bytes).  The backward pass is that of PEVIT_W_FP8_E4M3 (bf16 activations, saved in
                             bf16).  Deviation from the bf16-on-de-quantised run: profiles/r03_fp8_act.md.                */
    PEVIT_W_F32_VERIFY = 2 /* f32-class VERIFICATION mode, not a production format: weights and every activation kept in
                             f32, the matrix-core contractions run as plain f32 kernels (csrc/verify.hip) inside the same
                             launch sequences, layouts and index arithmetic.  Used by the parity tests to assert the stated
                             gates against the reference's fixtures without bf16 operand rounding; ~20x slower; workspace
                             and arena are twice the size.  All methods.                                                */
};

typedef struct pevit_dims {
    int32_t width;       /* E: visual.conv1.weight.shape[0]                 (model.py:1214) */
    int32_t layers;      /* L                                               (model.py:1215) */
    int32_t patch;       /* P                                               (model.py:1216) */
    int32_t resolution;  /* R = P * grid                                    (model.py:1218) */
    int32_t out_dim;     /* D: visual.proj.shape[1]                                         */
    int32_t method;      /* enum pevit_method                                               */
    int32_t lora_rank;   /* r (reference hard-codes 4: lora_model.py:461)                   */
    int32_t num_classes; /* C: DATASET.NUM_CLASSES          (kadaptation_clip.py:125)       */
    int32_t weight_format; /* enum pevit_weight_format                                      */
} pevit_dims;

const char* pevit_last_error(void);
int pevit_version(void);

int pevit_ctx_create(const pevit_dims* dims, pevit_ctx** out);
void pevit_ctx_destroy(pevit_ctx* ctx);

/* sizes the caller must provide */
size_t pevit_arena_bytes(const pevit_ctx* ctx);                 /* frozen weights, engine layout */
size_t pevit_workspace_bytes(const pevit_ctx* ctx, int batch);  /* activations + scratch          */
/* the leading bytes of the workspace that carry state from one launch to the next: the stream-K hand-off flags, the error word and
 * the skipped-update counter.  pevit_bind zeroes them and every launch leaves the flags zero again; the same for every batch and
 * for both layouts.  Everything behind them is scratch that every call writes before it reads: a caller may overwrite it between
 * two calls (not between a forward and the backward that runs on its saved activations). */
size_t pevit_workspace_state_bytes(const pevit_ctx* ctx);
/* number of f32 trainable parameters: tower adapters (reference named_parameters() order,
 * README.md:84-87 counts) followed by the head weight (C x D) and bias (C) */
size_t pevit_num_tower_params(const pevit_ctx* ctx);
size_t pevit_num_params(const pevit_ctx* ctx);
/* mask[i] = 1 if parameter i ever receives a gradient; 0 for the v_proj_adapter1_* tensors
 * of KAdaptation, which the reference never uses (model.py:580) and whose .grad stays None */
int pevit_param_grad_mask(const pevit_ctx* ctx, unsigned char* host_mask, size_t n);

int pevit_bind(pevit_ctx* ctx, void* arena, size_t arena_bytes, void* workspace, size_t workspace_bytes,
               int max_batch);
/* flat f32 parameter / gradient / momentum buffers (device, borrowed); gradients are
 * accumulated into `grads`.  `grad_mask` is the device copy of pevit_param_grad_mask (may be
 * NULL = every parameter is updated). */
int pevit_set_params(pevit_ctx* ctx, float* params, float* grads, float* momentum,
                     const unsigned char* grad_mask);

/* frozen weights: device f32 pointers in the OpenAI state-dict layout.  With fp8 weights pevit_load_block uses
 * the bound workspace as packing scratch: call it after pevit_bind, on the stream the context trains on, and not between a
 * forward and its backward (the saved activations are invalidated: the next backward without a new forward fails). */
int pevit_load_block(pevit_ctx* ctx, void* stream, int layer, const float* in_proj_weight,
                     const float* in_proj_bias, const float* out_proj_weight, const float* out_proj_bias,
                     const float* ln_1_weight, const float* ln_1_bias, const float* c_fc_weight,
                     const float* c_fc_bias, const float* c_proj_weight, const float* c_proj_bias,
                     const float* ln_2_weight, const float* ln_2_bias);
int pevit_load_stem(pevit_ctx* ctx, void* stream, const float* conv1_weight, const float* class_embedding,
                    const float* positional_embedding, const float* ln_pre_weight, const float* ln_pre_bias,
                    const float* ln_post_weight, const float* ln_post_bias, const float* proj);
/* Compacter's frozen shared phm_rule (4,4,4) (compacter_model.py:511-519) */
int pevit_load_phm_rule(pevit_ctx* ctx, void* stream, const float* phm_rule);

/* ---- the hot path ------------------------------------------------------------------ */
int pevit_transformer_forward(pevit_ctx* ctx, void* stream, const float* x_nbe, float* y_nbe, int batch,
                              int save_for_backward);
int pevit_transformer_backward(pevit_ctx* ctx, void* stream, const float* dy_nbe, float* dx_nbe_or_null,
                               int batch);
/* blocks [l_lo, l_hi) only -- ResidualAttentionBlock.forward (model.py:972-975) for l_hi = l_lo + 1, MultiheadAttention.forward
 * (model.py:837) being the attention half of it; pevit_transformer_* = the range [0, layers).  Every block keeps its own saved
 * activations: the blocks may be walked one call at a time and differentiated in reverse order (a walk starts at block 0). */
int pevit_blocks_forward(pevit_ctx* ctx, void* stream, const float* x_nbe, float* y_nbe, int batch, int save_for_backward,
                         int l_lo, int l_hi);
int pevit_blocks_backward(pevit_ctx* ctx, void* stream, const float* dy_nbe, float* dx_nbe_or_null, int batch, int l_lo,
                          int l_hi);
/* MultiheadAttention.forward(x, x, x, need_weights, attn_mask=None, average_attn_weights) of block `layer`
 * (model.py:837-944): x_nbe (N,B,E) f32 is the attention INPUT (ln_1's output inside the block); y_nbe (N,B,E) f32 is
 * out_proj(attention) WITHOUT the residual.  weights_or_null: (B,N,N) (average_weights = 1) or (B,H,N,N) (0) f32
 * softmax probabilities; NULL means need_weights = False.  The activations live in the layer's saved slots: a later
 * pevit_blocks_backward is refused, and so is a pevit_attention_backward after any other forward.  Weight formats bf16,
 * fp8 and f32-verify (fp8-act is refused). */
int pevit_attention_forward(pevit_ctx* ctx, void* stream, int layer, const float* x_nbe, float* y_nbe, int batch,
                            int save_for_backward, float* weights_or_null, int average_weights);
/* dy -> dx (may be NULL); accumulates the adapter gradients of `layer` into the flat gradient buffer, including
 * its share of the shared phm_rule factors, exactly as pevit_blocks_backward over [layer, layer+1) does.  Adapter,
 * Compacter and the frozen tower: stock attention with frozen weights, dx only (no gradient is written). */
int pevit_attention_backward(pevit_ctx* ctx, void* stream, int layer, const float* dy_nbe, float* dx_nbe_or_null,
                             int batch);
int pevit_visual_forward(pevit_ctx* ctx, void* stream, const float* images, float* feat, int batch,
                         int save_for_backward);
int pevit_visual_backward(pevit_ctx* ctx, void* stream, const float* dfeat, int batch);
/* the same backward cut at a block boundary: blocks layer_hi-1 .. layer_lo, whose adapter gradients are complete in
 * the flat buffer when the call's work has run (data parallelism all-reduces them while the next part runs).  The part
 * with layer_hi == layers takes dfeat; parts must be issued top-down and cover [0, layers) exactly once.  The shared
 * phm_rule gradients (KAdaptation) are complete after the part with layer_lo == 0. */
int pevit_visual_backward_part(pevit_ctx* ctx, void* stream, const float* dfeat_or_null, int batch, int layer_hi,
                               int layer_lo);
/* float offset of block `layer`'s parameters in the flat buffer (layer == layers: the head weight) */
size_t pevit_param_layer_offset(const pevit_ctx* ctx, int layer);
/* BatchNorm1d(D, affine=False) -> Linear(D, C) -> mean cross-entropy, forward + backward.
 * bn_training: batch statistics + running-stat update (momentum 0.1); else running stats.
 * Writes logits (B x C), loss (1), dfeat (B x D); accumulates head grads into the flat buffer.
 * Its scratch sits in the head slots of the layout the last saving forward left, so that the backward of that forward still finds
 * its activations; a batch LARGER than that forward's does not fit there: the workspace is laid out for it, and a backward through
 * the smaller forward is refused from then on. */
int pevit_head_forward_backward(pevit_ctx* ctx, void* stream, const float* feat, const int64_t* labels,
                                float* running_mean, float* running_var, int bn_training, float* logits,
                                float* loss, float* dfeat_or_null, int batch);
int pevit_zero_grads(pevit_ctx* ctx, void* stream);
/* flags: bit 0 = first step of the run (momentum buffer := gradient, like torch), bit 1 = Nesterov momentum */
int pevit_sgd_step(pevit_ctx* ctx, void* stream, float lr, float momentum, float weight_decay,
                   float grad_scale, int flags);
/* The fused update for the other optimizers optim/build.py constructs (build.py:107-170): torch.optim.Adam, torch.optim.AdamW
 * (torch 2.10, foreach=False: _single_tensor_adam) and torch.optim.SGD whose parameter groups differ in lr / weight decay.  One
 * launch over the flat buffer; plain SGD keeps pevit_sgd_step.
 * pevit_set_optim_state: device buffers of pevit_num_params elements (borrowed).  `group_of[i]` is the index of element i's
 * group in the `groups` array of pevit_optim_step; 255 = the parameter's .grad is None (nothing of it is touched, AdamW's
 * decoupled decay included) -- it takes the place of grad_mask here.  `exp_avg_sq` may be NULL while only the SGD kind is used;
 * exp_avg is the momentum buffer of pevit_set_params.
 * pevit_optim_group: plain floating-point values, in double: Python's scalars arrive unrounded, and everything derived from them
 * (1 - beta1, 1 - beta2, 1 - lr * wd, lr / (1 - beta1^step), sqrt(1 - beta2^step)) is computed in double and rounded to f32 once,
 * as torch does with its Python scalars.  The groups travel by value in the kernel arguments: no copy to the device.
 * pevit_optim_step: `step` is the 1-based count of updates (Adam kinds: the bias corrections); flags bit 0 = first step of the
 * run (SGD kind: momentum buffer := gradient, as for pevit_sgd_step).  Fails, launching nothing, when n_groups is outside
 * [1, PEVIT_OPTIM_MAX_GROUPS], step < 1 for the Adam kinds, the state is missing or the context has no parameters.  The
 * stream-K error word and pevit_set_external_poison withhold the update exactly as for pevit_sgd_step. */
enum pevit_optim_kind { PEVIT_OPTIM_SGD = 0, PEVIT_OPTIM_ADAM = 1, PEVIT_OPTIM_ADAMW = 2 };
#define PEVIT_OPTIM_MAX_GROUPS 8
typedef struct pevit_optim_group {
    double lr, weight_decay, momentum, beta1, beta2, eps;
    int nesterov;
} pevit_optim_group;
int pevit_set_optim_state(pevit_ctx* ctx, float* exp_avg_sq_or_null, const unsigned char* group_of);
int pevit_optim_step(pevit_ctx* ctx, void* stream, int kind, const pevit_optim_group* groups, int n_groups, int step,
                     float grad_scale, int flags);
/* uint8 pixels (B,3,R,R) instead of preprocessed f32: the dataset transforms of the reference (ToTensor + Normalize with
 * INPUT.MEAN / INPUT.STD: feature.py:537-542, resources/model/vitb32_CLIP.yaml:4-6), x = (u8 / 255 - mean[c]) / std[c], run inside
 * the patch gather -- bit for bit the f32 values `(x.float() / 255 - mean) / std` gives on the host; a quarter of the bytes
 * to upload.  pevit_set_input_norm must have been called on the context. */
int pevit_set_input_norm(pevit_ctx* ctx, const float* mean3, const float* std3);
int pevit_visual_forward_u8(pevit_ctx* ctx, void* stream, const uint8_t* images, float* feat, int batch, int save_for_backward);
int pevit_train_forward_backward_u8(pevit_ctx* ctx, void* stream, const uint8_t* images, const int64_t* labels,
                                    float* running_mean, float* running_var, int bn_training, float* logits,
                                    float* loss, int batch);
/* ---- native-size uint8 images: the reference's Resize(n_px, bicubic) + CenterCrop (clip_load.py:80-87) on the GPU, bit for bit
 * what Pillow's 8-bit resize gives, so that a dataset of 32 x 32 or 96 x 96 pixels is stored, kept resident and uploaded at its own
 * size and every _u8 entry above and below is fed from one launch.  Pillow's algorithm is exact integer arithmetic: per axis a table
 * of taps with 22 fractional bits, a horizontal pass rounded to uint8, a vertical pass over those bytes.  None of the three entries
 * takes a context; the two planners are host code and run without a GPU.
 * pevit_resize_geometry: a source of src_h rows and src_w columns and the target n_px -> the resized size (the shorter side becomes
 * n_px, the other int(n_px * longer / shorter)) and the crop window's first row and column, round((size - n_px) / 2) with halves
 * to the even neighbour like Python's round.
 * pevit_resize_axis: rows first .. first + count of the tables of one axis in_size -> out_size.  k (count x ksize) int32 taps, zero past
 * a row's tap count; bounds (count x 2) int32 = (first source sample, taps).  With k and bounds both null it returns ksize
 * (2 ceil(2 max(in_size / out_size, 1)) + 1; 1 for in_size == out_size) and writes nothing; otherwise 0.  An axis of equal size is
 * not resampled (Pillow skips that pass, and a bicubic pass at equal size is not the identity): its rows are the one tap 2^22 at the
 * sample itself.  The doubles are Pillow's, in Pillow's order, without contraction.
 * pevit_resize_u8: ONE launch, uint8 (planes x src_h x src_w) -> uint8 (planes x out_h x out_w), planes = 3 B, both dense, from
 * DEVICE tables kh (out_w x ksize_h), bh (out_w x 2), kv (out_h x ksize_v), bv (out_h x 2).  The centre crop is the window of table
 * rows handed in (rows left .. left + n_px of the horizontal axis, top .. top + n_px of the vertical one): no discarded pixel is
 * computed.  The intermediate of the horizontal pass lives in LDS only.  Source bytes are read one by one: no alignment is asked of
 * src, and nothing past its last pixel is touched.  Table contents are clamped on the device, so a wrong table gives wrong pixels
 * and never an access outside the buffers.  Limits, refused before any launch: 1 <= src_h, src_w <= 4096; 1 <= out_h, out_w <= 256;
 * 1 <= ksize_h, ksize_v <= 33 (a downscale of at most 8x); planes >= 1; no null pointer.  A plane's bytes do not depend on the other
 * planes of the launch. */
int pevit_resize_geometry(int src_h, int src_w, int n_px, int* nh, int* nw, int* top, int* left);
int pevit_resize_axis(int in_size, int out_size, int first, int count, int32_t* k, int32_t* bounds);
int pevit_resize_u8(void* stream, const uint8_t* src, int planes, int src_h, int src_w, uint8_t* dst, int out_h, int out_w,
                    const int32_t* kh, const int32_t* bh, int ksize_h, const int32_t* kv, const int32_t* bv, int ksize_v);
/* ---- ragged sets: every image its own size (Caltech-101, Pets, Flowers-102, ...), resized in ONE launch per batch.  The set is a
 * pool of dense (3, h_i, w_i) uint8 blocks that follow one another; one descriptor per image names its block and its tables; the
 * tables of all images live in two pools, one pair of out rows per distinct axis (in_size, out_size, first), planned by
 * pevit_resize_axis.  Centre crop or squash to out x out (DATASET.CENTER_CROP False) is only the choice of tables.
 * pevit_resize_ragged_desc: offset = byte offset of the block in the pool; h, w; kh_off / kv_off = element offsets into k_pool of the
 * axis' (out x ksize) int32 taps; bh_off / bv_off = element offsets into b_pool of its (out x 2) int32 bounds; ksize_h / ksize_v.
 * pevit_resize_ragged_check: host only, no GPU -- validates n_images HOST descriptors before they are uploaded: offset + 3 h w inside
 * the pool, sides in [1, 4096], ksize in [1, 33], table ranges inside the pools, out in [1, 256]; -1 with a message naming the first
 * image and what is wrong with it.
 * pevit_resize_ragged_u8: ONE launch; dst (batch x 3 x out x out) uint8, dense; output image b is image index[b] of the set (device
 * int64; null: image b).  All pointers but the struct itself are device memory.  max_ksize_v: the largest ksize_v of desc (it sizes
 * the LDS).  Every index the kernel forms is clamped -- image index, block, sides, ksize, table ranges, table contents, LDS rows --
 * so a wrong descriptor gives wrong pixels, never an access outside a buffer.  Refused before any launch: a null pointer (index
 * excepted), batch < 1, n_images < 1, out outside [1, 256], max_ksize_v outside [1, 33], pools smaller than one 1 x 1 image and one
 * one-tap table.  An image's bytes do not depend on the other images of the launch, and equal pevit_resize_u8's for the same tables. */
typedef struct pevit_resize_ragged_desc {
    int64_t offset;
    int32_t h, w;
    int32_t kh_off, bh_off, ksize_h;
    int32_t kv_off, bv_off, ksize_v;
} pevit_resize_ragged_desc;                        /* 40 bytes */
typedef struct pevit_resize_ragged_args {
    const uint8_t* pool; int64_t pool_bytes;
    const pevit_resize_ragged_desc* desc;
    const int32_t* k_pool; int64_t k_len;          /* lengths in int32 elements */
    const int32_t* b_pool; int64_t b_len;
    const int64_t* index; uint8_t* dst;
    int32_t n_images, batch, out, max_ksize_v;
} pevit_resize_ragged_args;
int pevit_resize_ragged_check(const pevit_resize_ragged_desc* host_desc, int n_images, int64_t pool_bytes, int64_t k_len,
                              int64_t b_len, int out);
int pevit_resize_ragged_u8(void* stream, const pevit_resize_ragged_args* args);
/* ---- evaluation: images (B,3,R,R) -> logits (B x C) in one call.  stem -> blocks -> ln_post -> proj -> BatchNorm1d(affine=False) in
 * EVAL mode on the caller's running statistics -> Linear.  The tower runs its inference forms: the kernels of pevit_visual_forward
 * with every store left out that only a backward pass reads (q' / v', log-sum-exp, the MLP pre-activation, LayerNorm statistics) and
 * one set of activation slots for all layers; features and logits are bit-identical to pevit_visual_forward(save_for_backward = 0)
 * followed by pevit_head_forward_backward(labels = NULL, bn_training = 0).  Reads the parameters and the running statistics; writes
 * logits, feat_or_null (B x D) and workspace scratch only -- not the gradient buffer, not the loss slot.  Like every forward it
 * leaves no saved forward behind: a backward issued afterwards is refused.  batch in [1, max_batch] of the bound workspace. */
int pevit_predict(pevit_ctx* ctx, void* stream, const float* images, const float* running_mean, const float* running_var,
                  float* logits, float* feat_or_null, int batch);
int pevit_predict_u8(pevit_ctx* ctx, void* stream, const uint8_t* images, const float* running_mean, const float* running_var,
                     float* logits, float* feat_or_null, int batch);   /* needs pevit_set_input_norm */
/* ---- zero-shot classification (commands/zeroshot.py, clip_zeroshot_evaluator.py:16-20 of the reference): images -> features, and
 * images -> class probabilities softmax(scale * normalize(features) @ text) in one call.
 * pevit_encode_image: the tower in the inference forms of pevit_predict, without a head -- CLIP.encode_image for evaluation; the
 * features are the bits pevit_predict returns in feat_or_null.
 * pevit_zeroshot: the same walk, then ONE launch of the zero-shot head on the features: s_b = scale / max(||feat_b||_2, 1e-12) (the
 * eps clamp of F.normalize), logits[b][c] = s_b * <feat_b, text_c>, probs[b][:] = softmax(logits[b][:]) with the row maximum
 * subtracted -- all f32 on the f32 matrix instruction, no bf16 rounding.  text_cd: device f32 (num_classes x D), CLASS-major, one
 * unit vector per row (the transpose of the reference's (D, C) text_features, made once per evaluation); num_classes is
 * independent of pevit_dims.num_classes.  probs_or_null / logits_or_null: (batch x num_classes) f32, either may be null, not both;
 * feat_or_null: (batch x D), or null to keep the features in workspace scratch.  Every reduction of the head runs in a fixed order
 * that depends on D and num_classes only, so a row's outputs are bit-identical alone and inside any batch; a zero feature row gives
 * uniform probabilities.  Limits: 1 <= num_classes <= 1024, D a multiple of 8 up to 1024, text_cd (and feat) 16-byte aligned;
 * anything else is refused before any launch.  All four read the parameters and write their outputs and workspace scratch only;
 * they leave no saved forward behind (a backward issued afterwards is refused), work with every method (PEVIT_NONE is the plain
 * CLIP the reference scores) and every weight format, refuse a text context and an unbound one, and take batch in
 * [1, max_batch] of the bound workspace.  The _u8 forms need pevit_set_input_norm. */
int pevit_encode_image(pevit_ctx* ctx, void* stream, const float* images, float* feat, int batch);
int pevit_encode_image_u8(pevit_ctx* ctx, void* stream, const uint8_t* images, float* feat, int batch);
int pevit_zeroshot(pevit_ctx* ctx, void* stream, const float* images, const float* text_cd, int num_classes, float scale,
                   float* probs_or_null, float* logits_or_null, float* feat_or_null, int batch);
int pevit_zeroshot_u8(pevit_ctx* ctx, void* stream, const uint8_t* images, const float* text_cd, int num_classes, float scale,
                      float* probs_or_null, float* logits_or_null, float* feat_or_null, int batch);
/* ---- serving: an image context that can ONLY infer, next to a frozen tower, with adapters swapped in by pointer.
 * pevit_infer_create: the checks and errors of pevit_ctx_create for every method and weight format; dims->num_classes is the LARGEST
 * head the context will serve (it sizes the logits slot).  Its arena holds what the inference walk reads and nothing else: no
 * transposed copy of a frozen matrix (the dX operands of a backward), no proj as the backward reads it; one write-only [width][64]
 * panel per layer takes the transposed adapter panels that the panel-building kernels store whoever runs them.  Its workspace
 * (pevit_workspace_bytes) is a third layout: the state words and the stream-K slabs, ONE set of per-layer activation slots without
 * LayerNorm statistics and without the MLP pre-activation plus the alternate block input, the final residual stream, the ln_2
 * output, gelu(h) (and the two e4m3 copies of fp8-act), one [tokens][width] f32 scratch, and the stem / feature / eval-head slots
 * -- nothing that only a backward, a gradient reduction or a training head touches; its size does not depend on the layer count.
 * pevit_bind, pevit_load_block (which needs no workspace scratch here, in any format), pevit_load_stem, pevit_load_phm_rule,
 * pevit_set_input_norm, pevit_predict[_u8], pevit_encode_image[_u8], pevit_zeroshot[_u8] and the size / status / tune / profile
 * queries run on it, with the kernels and the bits of the same call on a pevit_ctx_create context.  Every other entry point that
 * takes a context is refused on the host before any launch ("inference-only context" in pevit_last_error); the workspace and its
 * flag words are left alone.
 * pevit_set_infer_params: params = device f32 [tower adapters in the flat order of pevit_set_params | head W (num_classes x D) | head b
 * (num_classes)], 1 <= num_classes <= dims.num_classes; only read.  The head offsets and pevit_num_params follow num_classes, and
 * pevit_predict writes batch x num_classes logits from then on.  Calling it again swaps the adapter: the walk rebuilds the adapter
 * panels from this buffer on every forward, so a swap costs nothing else.  The buffer must stay alive while it is set. */
int pevit_infer_create(const pevit_dims* dims, pevit_ctx** out);
int pevit_set_infer_params(pevit_ctx* ctx, const float* params, int num_classes);
/* the zero-shot head alone, context-free (parity tests): feat (B x D), text_cd (C x D), outputs (B x C) */
int pevit_op_zeroshot_head(void* stream, const float* feat, const float* text_cd, float scale, float* probs_or_null,
                           float* logits_or_null, int B, int D, int C);
/* ---- the linear probe on CACHED features (evaluation/full_model_finetune.py with FREEZE_IMAGE_BACKBONE: nothing below the head
 * trains, so every image needs the tower once per checkpoint -- pevit_encode_image -- and every step and every validation after
 * that is head-only work on rows of a feature matrix).  Both entries need a bound image context of method PEVIT_NONE with
 * parameters set (pevit_set_params: the head weight [C][D] and bias [C] are the whole flat buffer); a text context, another
 * method and an unbound context are refused.  Limits, refused before any launch: D (pevit_dims.out_dim) a multiple of 16 up to
 * 1024, num_classes <= 1024, feat 16-byte aligned.
 * pevit_probe_step: ONE training step as two launches.  x = feat[index[b]] (index values are clamped to [0, rows) on the device),
 * logits = scale * (BatchNorm1d(x) W^T + bias) in exact f32 (scale = exp(logit_scale), frozen: reference line 156; 1 for the plain
 * head), mean cross-entropy over labels[index[b]] (int64, ignore_index -100 as torch) or mean BCE-with-logits over
 * targets[index[b]][:] (f32) -- exactly one of labels / targets.  bn_training: batch statistics + PyTorch's running-statistics
 * update (unbiased variance, momentum 0.1, eps 1e-5), else the running statistics.  The head's gradients are WRITTEN to the
 * gradient buffer (pevit_zero_grads is not needed before).  update != 0: torch.optim.SGD on the head inside the second launch
 * with lr / momentum / weight_decay and the flags of pevit_sgd_step (bit 0 first step, bit 1 Nesterov); the stream-K and external
 * error words do not gate it (no stream-K product ran).  update == 0: parameters and momentum are untouched and the caller follows
 * with pevit_optim_step.  Writes logits (batch x C) and loss (1), which may be rows of the caller's epoch buffers.
 * 2 <= batch <= max_batch of the bound workspace (its head slots hold the hand-over between the two launches; a saved forward is
 * dropped).  Every reduction runs in a fixed order: the same call from the same state gives the same bits.
 * pevit_probe_predict: logits = scale * (BatchNorm1d_eval(x) W^T + bias) for `count` rows in ONE launch: x = feat[index[i]], or
 * feat[first_row + i] with a null index.  count >= 1 is not bounded by max_batch (nothing is staged in the workspace); a row's
 * bits do not depend on the other rows of the call.  Reads parameters and running statistics, writes logits (count x C) only. */
typedef struct pevit_probe_args {
    const float* feat; int64_t rows;           /* cached features (rows x D) */
    const int64_t* index;                      /* (batch) rows of feat */
    const int64_t* labels;                     /* (rows) class indices, or NULL */
    const float* targets;                      /* (rows x C) multi-hot / soft targets, or NULL */
    float* running_mean; float* running_var;   /* (D) */
    float* logits; float* loss;                /* (batch x C), (1) */
    int batch, bn_training, update, flags;
    float scale, lr, momentum, weight_decay;
} pevit_probe_args;
int pevit_probe_step(pevit_ctx* ctx, void* stream, const pevit_probe_args* args);
typedef struct pevit_probe_predict_args {
    const float* feat; int64_t rows;
    const int64_t* index_or_null; int64_t first_row; int count;
    const float* running_mean; const float* running_var;
    float scale;
    float* logits;                             /* (count x C) */
} pevit_probe_predict_args;
int pevit_probe_predict(pevit_ctx* ctx, void* stream, const pevit_probe_predict_args* args);
/* ---- the CLIP text tower (CLIP.encode_text, model.py:1153-1168): token ids (S x N) int64 -> text features (S x D) f32 in one call.
 * A text context is a pevit_ctx like any other -- method PEVIT_NONE, H = width / 64 heads, N = context_length tokens per prompt,
 * causal attention -- so pevit_arena_bytes, pevit_bind, pevit_load_block (q rows pre-scaled by 1/8 as for the image tower) and
 * pevit_ctx_destroy work on it unchanged.  It is inference-only: pevit_workspace_bytes returns the size of the inference layout
 * (one set of activation slots for all layers) and max_batch of pevit_bind counts PROMPTS.  Limits: width a multiple of 128 up to
 * 1024, out_dim a multiple of 8, 1 <= context_length <= 128, weight_format PEVIT_W_BF16 or PEVIT_W_F32_VERIFY (the fp8 formats
 * are refused).  Every image-side and training entry point refuses a text context with a message, and pevit_encode_text refuses
 * an image context. */
typedef struct pevit_text_dims {
    int32_t width, layers, context_length, vocab_size, out_dim, weight_format;
} pevit_text_dims;
int pevit_text_create(const pevit_text_dims* dims, pevit_ctx** out);
/* device pointers, f32: token_embedding [V][E] (kept f32 in the arena: the embedding is exact), positional_embedding [N][E],
 * ln_final weight / bias [E], text_projection [E][D] */
int pevit_load_text_stem(pevit_ctx* ctx, void* stream, const float* token_embedding, const float* positional_embedding,
                         const float* ln_final_weight, const float* ln_final_bias, const float* text_projection);
/* embed -> the L blocks in their inference forms with causal attention -> the row of each prompt's FIRST largest token id (the
 * end-of-text marker; torch.argmax) through ln_final -> @ text_projection.  tokens: device int64 [prompts][N]; ids outside
 * [0, V - 1] are clamped by the embedding kernel (callers check the range).  prompts in [1, max_batch]; larger sets are split
 * by the caller. */
int pevit_encode_text(pevit_ctx* ctx, void* stream, const int64_t* tokens, float* features, int prompts);
/* whole fine-tune step: zero_grad -> forward -> CE -> backward -> (caller all-reduces) -> SGD */
int pevit_train_forward_backward(pevit_ctx* ctx, void* stream, const float* images, const int64_t* labels,
                                 float* running_mean, float* running_var, int bn_training, float* logits,
                                 float* loss, int batch);
/* ---- multi-label: the three entries above with BCEWithLogitsLoss(reduction="mean") in place of the cross-entropy.
 * targets: f32 (B x C) row-major, multi-hot or soft; loss = sum(l) / (B*C) with l = max(x,0) - x*y + log1p(exp(-|x|)),
 * dlogits = (sigmoid(x) - y) / (B*C).  Everything else -- BatchNorm, the head gradients, dfeat, the tower backward, the loss
 * slot that a withheld update overwrites with NaN -- is what the cross-entropy entries do. */
int pevit_head_forward_backward_bce(pevit_ctx* ctx, void* stream, const float* feat, const float* targets,
                                    float* running_mean, float* running_var, int bn_training, float* logits,
                                    float* loss, float* dfeat_or_null, int batch);
int pevit_train_forward_backward_bce(pevit_ctx* ctx, void* stream, const float* images, const float* targets,
                                     float* running_mean, float* running_var, int bn_training, float* logits,
                                     float* loss, int batch);
int pevit_train_forward_backward_bce_u8(pevit_ctx* ctx, void* stream, const uint8_t* images, const float* targets,
                                        float* running_mean, float* running_var, int bn_training, float* logits,
                                        float* loss, int batch);

/* ---- measurement: HIP events around every MFMA GEMM launch of the context (the dominant kernel
 * family); totals over the GEMM launches recorded between begin and end.  With pevit_tune(ctx, "profile_all", 1) the
 * HBM-bound kernels of the step are bracketed as well: their records carry epi_mnk[0] = 100 + pevit_prof_kind, the row
 * count in epi_mnk[1], flops 0 and their algorithmic bytes; *launches counts every record, the totals only the GEMMs. */
enum pevit_prof_kind {
    PEVIT_PROF_LN_FWD = 0, PEVIT_PROF_LN_BWD = 1, PEVIT_PROF_ATTN_FWD = 2, PEVIT_PROF_ATTN_BWD = 3, PEVIT_PROF_DELTA_ADD = 4,
    PEVIT_PROF_LOWRANK_U = 5, PEVIT_PROF_LOWRANK_GRAD = 6, PEVIT_PROF_IM2COL = 7, PEVIT_PROF_LOWRANK_BWD = 8,
    PEVIT_PROF_ATTN_FWD_DELTA = 9, PEVIT_PROF_ADAPTER_FWD = 10, PEVIT_PROF_ADAPTER_BWD = 11,
    PEVIT_PROF_GRAD_SUMSQ = 12, PEVIT_PROF_GRAD_SCALE = 13
};
int pevit_profile_begin(pevit_ctx* ctx, int max_launches);
int pevit_profile_end(pevit_ctx* ctx, double* total_ms, double* total_flops, double* total_bytes, int* launches);
/* launch i (0 <= i < *launches of the last pevit_profile_end): its duration, 2*M*N*K and {epilogue, M, N, K} */
int pevit_profile_launch(pevit_ctx* ctx, int i, double* ms, double* flops, int* epi_mnk);
/* ... and the bytes it must move at least: every operand read once, every result written once */
int pevit_profile_launch_bytes(pevit_ctx* ctx, int i, double* bytes);

/* ---- single kernels, exposed for parity tests and profiling ------------------------- */
int pevit_op_gemm(void* stream, int epilogue, const void* A_bf16, int lda, const void* B_bf16, int ldb, int b_rows,
                  int M, int N, int K, const float* bias, const float* resid, int ldr, float* out_f32, int ldo,
                  void* out_bf16, int ldob, void* out2_bf16, int ldob2, const void* aux_bf16, int ldaux,
                  size_t head_stride, int E, int H, int tokens);
/* fp8 weights (PEVIT_W_FP8_E4M3): B = e4m3 codes [b_rows][ldb] as written by pevit_op_quant_fp8 (k-permuted per 128),
 * bscale = per-output-column scale applied to the accumulator (NULL: none), oscale = per-column factor folded into the
 * bf16 output of the DGELU epilogue (NULL: none); K % 128 == 0.  Epilogues 0..5 only. */
int pevit_op_gemm_fp8(void* stream, int epilogue, const void* A_bf16, int lda, const void* B_codes, int ldb, int b_rows,
                      const float* bscale, const float* oscale, int M, int N, int K, const float* bias,
                      const float* resid, int ldr, float* out_f32, int ldo, void* out_bf16, int ldob, void* out2_bf16,
                      int ldob2, const void* aux_bf16, int ldaux, size_t head_stride, int E, int H, int tokens);
/* fp8 x fp8 (PEVIT_W_FP8_ACT): A = UNSCALED saturating e4m3 codes [M][lda] (pevit_op_cast_fp8), B / bscale as above; the
 * matrix-core instruction is v_mfma_scale_f32_32x32x64_f8f6f4 with unit block scales.  Epilogues 0, 1, 2, 4; out2_fp8: the
 * EPI_BIAS_GELU activation output is written as e4m3 codes (ldob2 in codes). */
int pevit_op_gemm_f8a(void* stream, int epilogue, const void* A_codes, int lda, const void* B_codes, int ldb, int b_rows,
                      const float* bscale, int M, int N, int K, const float* bias, const float* resid, int ldr,
                      float* out_f32, int ldo, void* out_bf16, int ldob, void* out2, int ldob2, int out2_fp8,
                      size_t head_stride, int E, int H, int tokens);
/* src (rows x cols f32, cols % 128 == 0) -> e4m3 codes without a scale (|x| > 448 saturates), k-permuted per 128 */
int pevit_op_cast_fp8(void* stream, const float* src, void* codes, int rows, int cols);
/* Which kernel family the last pevit_op_gemm / in-step product of this process was launched on (tests, measurements):
 * 1 plain tile, 2 staggered 8-wave tile, 3 k-split tile (alternate k-tiles), 4 phased k-split tile, 5 stream-K, 6 few-row split-K. */
int pevit_debug_last_gemm_path(void);
/* W (rows x cols f32, cols % 128 == 0) -> per-row power-of-two scales 2^ceil(log2(amax/448)), e4m3 codes [rows][cols]
 * and (codes_t != NULL, rows % 128 == 0) the same codes transposed [cols][rows]; both k-permuted per 128 */
int pevit_op_quant_fp8(void* stream, const float* W, int rows, int cols, void* codes, float* scales, void* codes_t);
int pevit_op_dequant_fp8(void* stream, const void* codes, const float* scales, int rows, int cols, float* out_f32);
int pevit_op_ln_fwd(void* stream, const float* x, const float* gamma, const float* beta, int rows, int E,
                    void* y_bf16, float* y_f32, float* mean, float* rstd);
int pevit_op_ln_bwd(void* stream, const float* dy, const float* x, const float* mean, const float* rstd,
                    const float* gamma, const float* dres, float* dx, void* dx_bf16, int rows, int E);
/* as pevit_op_ln_bwd, with a per-column factor on the bf16 copy only (fp8 weights: channel scales of the consuming GEMM) */
int pevit_op_ln_bwd_scaled(void* stream, const float* dy, const float* x, const float* mean, const float* rstd,
                           const float* gamma, const float* dres, float* dx, void* dx_bf16, int rows, int E,
                           const float* bf16_colscale);
/* lse == NULL: the inference instance, which does not store the log-sum-exp (same out) */
int pevit_op_attn_fwd(void* stream, const void* q, const void* k, const void* v, void* out, int ldo, float* lse,
                      int B, int H, int N);
int pevit_op_attn_bwd(void* stream, const void* q, const void* k, const void* v, const void* out, int ldo,
                      const void* dout, int lddo, const float* lse, void* dqkv, int ld, int B, int H, int N);
/* causal attention of the text tower (query x sees the keys y <= x), forward only, 1 <= N <= 128: operands as pevit_op_attn_fwd,
 * no log-sum-exp */
int pevit_op_attn_fwd_causal(void* stream, const void* q, const void* k, const void* v, void* out, int ldo, int B, int H, int N);
int pevit_op_cast_bf16(void* stream, const float* src, void* dst, size_t n, float scale);
/* q16: Q as a bf16 panel [E][64] (Q_q | Q_v), the production operand of the forward delta */
int pevit_op_delta_add(void* stream, void* qbuf, void* vbuf, const float* t, const void* q16_bf16, const float* bias,
                       float ascale, int B, int N, int E);
/* delta_add + attn_fwd as ONE launch (attn_delta.hip) for geometries where pevit_op_attn_delta_hpw(B, H, N) > 0 (runs of that
 * many heads own whole reference rows of the raw reshape, model.py:796-799; N <= 64): q and v are rewritten with q + delta,
 * v + delta; bit-identical to pevit_op_delta_add followed by pevit_op_attn_fwd.  lse == NULL: the inference instance -- q and v are
 * only read (q + delta, v + delta never leave the chip), no lse; the same out */
int pevit_op_attn_fwd_delta(void* stream, void* q, const void* k, void* v, const float* t, const void* q16_bf16, const float* bias,
                            float ascale, void* out, int ldo, float* lse, int B, int H, int N);
int pevit_op_attn_delta_hpw(int B, int H, int N);
/* The segmented forms of the two kernels above (pevit_segments.h: pevit_predict_segments), inference only.  The B images are split
 * into nseg <= 16 contiguous segments that tile [0, B) in order; the raw reshape of the delta works INSIDE a segment (local reference
 * row rr: token rr / count of image first + rr % count) with that segment's bf16 Q panel, bias (or NULL) and its 64 columns
 * [tcol, tcol + 64) of t, whose rows are tpitch floats apart (tpitch and tcol multiples of 64).  Each segment of the output is, bit
 * for bit, what the unsegmented entry gives on that segment's slices alone.
 *   delta_add_seg:      q and v (B*H, N, 64) are rewritten in place; pevit_op_attn_fwd follows unchanged
 *   attn_fwd_delta_seg: one launch where pevit_op_attn_delta_hpw(B, H, N) > 0; q and v are only read; one workgroup per run of heads
 *                       inside a segment, so the grid is sum_s ceil(count_s * H / 6) */
typedef struct pevit_op_segment {
    int32_t first, count, tcol;
    const void* q16_bf16;
    const float* bias;
} pevit_op_segment;
int pevit_op_delta_add_seg(void* stream, void* qbuf, void* vbuf, const float* t, int tpitch, float ascale, int B, int H, int N,
                           int nseg, const pevit_op_segment* segs);
int pevit_op_attn_fwd_delta_seg(void* stream, const void* q, const void* k, const void* v, const float* t, int tpitch, float ascale,
                                void* out, int ldo, int B, int H, int N, int nseg, const pevit_op_segment* segs);
/* softmax probabilities P = exp(q k^T - lse) (attn_probs.hip): q, k (B*H, N, 64) bf16 as pevit_op_attn_fwd takes them, lse as it
 * wrote it; average = 1: out (B, N, N) f32, the mean over the H heads; 0: out (B, H, N, N) f32.  N <= 384. */
int pevit_op_attn_probs(void* stream, const void* q, const void* k, const float* lse, float* out, int B, int H, int N, int average);
/* Test-only forms of the four entry points above (tests/test_gpu_kernel_forms.py): the members of the launchers' parameter structs
 * that only the training step sets, one kernel at a time.  They add no kernel; 0 / NULL in the extra arguments is the plain call.
 *   ln_fwd_ex:   xstride = elements between the rows of x (0: E); y_fp8 = k-permuted e4m3 copy [rows][E] (E % 128 == 0)
 *   ln_bwd_ex:   dy is f32, or (dy_stored) bf16; dres is f32, or (res16, needs dy_stored and dx_bf16) bf16 -- it may then be dx_bf16
 *                itself (in place) and dx may be NULL; res_period > 0: dres is read on rows that are multiples of it only (zero
 *                elsewhere); xstride = elements between the rows of x, dres, dx and dx_bf16 (dy, mean, rstd stay compact);
 *                bf16_colscale: power-of-two column factors on dx_bf16; res_colscale (res16): such factors taken out of dres
 *   attn_fwd_ex: out_fp8 = k-permuted e4m3 copy of out, row pitch ldo codes
 *   attn_bwd_ex: dout_cls_only (N <= 64) = dout is zero except on token 0 of every image, the other rows are not read */
int pevit_op_ln_fwd_ex(void* stream, const float* x, const float* gamma, const float* beta, int rows, int E, size_t xstride,
                       void* y_bf16, float* y_f32, float* mean, float* rstd, void* y_fp8);
int pevit_op_ln_bwd_ex(void* stream, const void* dy, int dy_stored, const float* x, const float* mean, const float* rstd,
                       const float* gamma, const void* dres, int res16, int res_period, float* dx, void* dx_bf16,
                       int rows, int E, size_t xstride, const float* bf16_colscale, const float* res_colscale);
int pevit_op_attn_fwd_ex(void* stream, const void* q, const void* k, const void* v, void* out, int ldo, float* lse,
                         int B, int H, int N, void* out_fp8);
int pevit_op_attn_bwd_ex(void* stream, const void* q, const void* k, const void* v, const void* out, int ldo,
                         const void* dout, int lddo, const float* lse, void* dqkv, int ld, int B, int H, int N,
                         int dout_cls_only);
/* Test-only form of the three GEMM entry points above (tests/test_gpu_gemm_forms.py): EVERY member of the launcher's parameter
 * struct, by name, from one flat argument struct -- the second f32 output of EPI_BIAS_RESID_KEEP (out_f32_2 / ldo2), the bf16 tail of
 * an fp8-B product (B2 / ldb2 / b2_rows / n_fp8: output columns >= n_fp8 take their B rows from B2, which lies behind B), the operand
 * forms (b_fp8, a_fp8, bscale, oscale) -- a tune of its own, and the caller's stream-K workspace.  It adds no kernel.
 *   tune:      a default-constructed tune in which the knobs whose bit is set in tune_set are overwritten (bit i = the i-th of
 *              config, stagger, big, ksplit, ksplit_small, ksplit_stagger, ksplit_mink, kphase_nl, kz2, skinny, skinny_slices,
 *              streamk, persistent: enum pevit_gemm_knob); the process-wide tune of pevit_tune(NULL, ...) is neither read nor written
 *   workspace: sk_flag = sk_slots + 1 zeroed words (hand-off flags / tickets, then the error word at sk_flag[sk_slots]), sk_slab =
 *              sk_slots x 128 x 128 floats, sk_slots = pevit_op_gemm_sk_slots(); all NULL / 0: the families that need one are not taken */
enum pevit_gemm_knob {
    PEVIT_KNOB_CONFIG = 0, PEVIT_KNOB_STAGGER = 1, PEVIT_KNOB_BIG = 2, PEVIT_KNOB_KSPLIT = 3, PEVIT_KNOB_KSPLIT_SMALL = 4,
    PEVIT_KNOB_KSPLIT_STAGGER = 5, PEVIT_KNOB_KSPLIT_MINK = 6, PEVIT_KNOB_KPHASE_NL = 7, PEVIT_KNOB_KZ2 = 8, PEVIT_KNOB_SKINNY = 9,
    PEVIT_KNOB_SKINNY_SLICES = 10, PEVIT_KNOB_STREAMK = 11, PEVIT_KNOB_PERSISTENT = 12, PEVIT_KNOB_COUNT = 13
};
typedef struct pevit_gemm_ex_args {
    const void* A; const void* B; const void* B2;
    const float* bias; const float* resid; const float* bscale; const float* oscale;
    float* out_f32; float* out_f32_2; void* out_bf16; void* out2_bf16; const void* aux_bf16;
    float* sk_slab; unsigned* sk_flag;
    size_t head_stride;
    int32_t epilogue, M, N, K;
    int32_t lda, ldb, b_rows, ldb2, b2_rows, n_fp8, b_fp8, a_fp8;
    int32_t ldr, ldo, ldo2, ldob, ldob2, ldaux;
    int32_t E, H, tokens, sk_slots;
    uint32_t tune_set;                      /* bit per knob of tune[] that is set */
    int32_t tune[13];                       /* indexed by enum pevit_gemm_knob */
} pevit_gemm_ex_args;
int pevit_op_gemm_ex(void* stream, const pevit_gemm_ex_args* args);
int pevit_op_gemm_sk_slots(void);           /* residency slots of the stream-K workspace on this device (pevit_op_gemm sizes its own by it) */
/* Debug seams of the GEMM planner (csrc/gemm_plan.hip), callable without a GPU: neither makes a HIP call or touches a pointer.
 *   pevit_debug_gemm_plan: the plan pevit_op_gemm_ex would launch for `args` on a device of `cus` compute units -- the kernel family
 *       (path, as pevit_debug_last_gemm_path), operand form, tile configuration and grid.  The planner reads pointers only as set /
 *       unset and as the B2 - B distance, so made-up non-null addresses do.  Returns 0 with err empty, or -1 with the planner's
 *       message in err and in pevit_last_error.
 *   pevit_debug_gemm_epi_traits: which families have an instantiation for an epilogue: bit 0 fp8 B, bit 1 fp8 x fp8, bit 2 the few-row
 *       kernel, bit 3 the k-split / phased k-split / stream-K kernels; -1 for an unknown epilogue */
typedef struct pevit_gemm_plan_info {
    int32_t path, ops, cfg, wm, nl, stag, tiles, grid, band, sk_share, sk_band, tiles_n, nslices, ksl;
    char err[160];
} pevit_gemm_plan_info;
int pevit_debug_gemm_plan(const pevit_gemm_ex_args* args, int cus, pevit_gemm_plan_info* out);
int pevit_debug_gemm_epi_traits(int epilogue);
/* Test-only form of the fused post-MLP adapter launches (adapter_fused.hip; tests/test_gpu_adapter_fused.py): EVERY member of the
 * launchers' parameter structs, by name, from one flat argument struct each (zero-initialised = nothing set).  They add no kernel.
 *   act_kind 0 = ReLU (Adapter), 1 = gelu_new (Compacter); E in {256, 512, 768, 1024} (pevit_op_adapter_fused_ok), T >= 1
 *   forward:  hraw [T][E] f32 = the c_proj accumulators WITHOUT their bias bpr [E]; x_mid [T][E] f32; gamma, beta [E]; wd [64][E] and
 *             wu [E][64] bf16; b_down [64], b_up [E] -> z [T][E] bf16, mean_a / rstd_a [T], act [T][64] bf16, apre [T][64] bf16
 *             (gelu_new only: the ReLU kernel does not touch it), x_out [T][E] f32
 *   backward: dyb [T][E] bf16 = dx_out; dres [T][E] f32 = dx_out, or NULL (the residual and the d b_up sums then take dyb);
 *             wuT [64][E], wdT [E][64] bf16; saved [T][64] bf16 = act (ReLU) / apre (gelu_new) -> dpre [T][64] bf16, dh_bf16 [T][E],
 *             partial [pevit_op_adapter_blocks(T)][3][E] = column sums of dz * xhat, dz, dx_out over the rows of each workgroup
 *   tn_*:     the token-contracted products that ride in the backward launch, layouts of pevit_op_tn_gemm64 below: product 1 =
 *             (tn_x1 [T][E], tn_y1 [T][64]) -> tn_partial1; product 2 = (tn_x2, tn_y2) -> tn_partial2 and the column sums of tn_y2
 *             -> tn_csy2; tn_x1 / tn_x2 NULL leave a product out; tn_y2 must not be dpre; tn_blocks = workgroups of that range
 *             (0: one per pair of (256-row chunk, 64-column slab) units) */
typedef struct pevit_adapter_fwd_args {
    const float* hraw; const float* bpr; const float* x_mid; const float* gamma; const float* beta;
    const void* wd; const float* b_down; const void* wu; const float* b_up;
    void* z; float* mean_a; float* rstd_a; void* act; void* apre; float* x_out;
    int32_t act_kind, T, E;
} pevit_adapter_fwd_args;
typedef struct pevit_adapter_bwd_args {
    const void* dyb; const float* dres; const void* wuT; const void* saved; const void* wdT;
    const float* hraw; const float* bpr; const float* mean_a; const float* rstd_a; const float* gamma;
    void* dpre; void* dh_bf16; float* partial;
    const void* tn_x1; const void* tn_y1; float* tn_partial1;
    const void* tn_x2; const void* tn_y2; float* tn_partial2; float* tn_csy2;
    int32_t act_kind, T, E, tn_blocks;
} pevit_adapter_bwd_args;
int pevit_op_adapter_fwd_ex(void* stream, const pevit_adapter_fwd_args* args);
int pevit_op_adapter_bwd_ex(void* stream, const pevit_adapter_bwd_args* args);
int pevit_op_adapter_blocks(int T);         /* workgroups (= blocks of `partial`) of the fused backward */
int pevit_op_adapter_fused_ok(int E);       /* 1: the fused launches take this width */
/* Test-only form of the segmented inference launch of the fused forward (adapter_fused.hip adapter_fwd_seg_kernel;
 * tests/test_gpu_segments_postmlp.py).  hraw, bpr, x_mid, x_out as above, over all rows; segs: a HOST array of nseg in [1,16]
 * segments, rows [first, end) each with its own gamma, beta [E], wd [64][E] and wu [E][64] bf16, b_down [64], b_up [E].  One launch of
 * sum_s ceil((end_s - first_s) / 32) workgroups, none of which crosses a segment end; x_out of a segment has the bits of
 * pevit_op_adapter_fwd_ex on that segment's rows alone.  Nothing else is written (no z, act, apre, mean_a, rstd_a). */
typedef struct pevit_adapter_seg {
    int32_t first, end;
    const float* gamma; const float* beta; const void* wd; const float* b_down; const void* wu; const float* b_up;
} pevit_adapter_seg;
typedef struct pevit_adapter_fwd_seg_args {
    const float* hraw; const float* bpr; const float* x_mid; float* x_out; const pevit_adapter_seg* segs;
    int32_t act_kind, E, nseg;
} pevit_adapter_fwd_seg_args;
int pevit_op_adapter_fwd_seg(void* stream, const pevit_adapter_fwd_seg_args* args);
/* Test-only forms of the attention-site low-rank adapter launches (lowrank.hip; tests/test_gpu_lowrank.py): the members of the
 * launchers' parameter structs, by name, from one flat argument struct each (zero-initialised = nothing set).  They add no kernel.
 *   pevit_op_lowrank_ex:    form = enum pevit_lowrank_form.  LOWRANK_U: dqkv [T][ld] bf16 (q | k | v gradients in row layout), qT
 *             [64][E] bf16 -> u32 [T][64] f32 and its bf16 copy at u_bf16_cols (row pitch ld).  LOWRANK_GRAD: xn [T][ldx] bf16, u32,
 *             dqkv, t [T][64] f32 -> partial [chunks][4][E][32], dbias_partial [chunks][2][E]; chunks = pevit_op_lowrank_chunks(B * N);
 *             xcd_order = the XCD-contiguous workgroup order.  LOWRANK_COMBO: u and dQ / d bias of this layer (this_layer) and the
 *             deferred dP = xn_prev^T u32_prev -> partial_prev (prev) in one launch.  LOWRANK_U_F32 / LOWRANK_GRAD_F32: the f32
 *             verification kernels; dqkv, u_bf16_cols and xn then hold f32 (ld, ldx in floats) and lowrank_u reads q32 [E][64].
 *   pevit_op_prep_lowrank:  the panels of `layers` layers from the f32 parameters.  method PEVIT_KADAPTATION: rule1_l .. rule2_r
 *             [32][32], q_left / q_right [32][E / 32] per layer; PEVIT_LORA: a1q, a1v [r][E], a2q, a2v [E][r] per layer.  Panels
 *             (kernels.h AdapterPanels): w_aug_rows [64][ldw], wT_aug_cols [E][ldwT] (64 columns written), qT [64][E], q16 [E][64]
 *             in bf16 (f32 = 1: in f32, q16 not written), q32 [E][64] f32.  Layer l reads its parameters param_floats * l floats
 *             and writes its panels arena_bytes * l bytes behind layer 0's.
 *   pevit_op_chain_lowrank: the reduce of the per-chunk partials and the chain rule onto the flat gradient buffer, as the backward
 *             walk fills ChainKadaptArgs / ChainLoraArgs (partial_layer, dbias_layer in floats; p_layer0 = first float of the first
 *             layer's parameters in params / grads, p_layer_stride floats between layers; params[0:4096] = the four rule factors).
 *             PEVIT_LORA takes no dbias_partial, rule_scratch or params.
 *   pevit_op_rule_sum:      grads[0:4096] += rule_scratch[l][0:4096] for l = l_hi - 1 .. l_lo
 *   pevit_op_lowrank_plan:  out = {es, nu, n12, n0, chunks} of the launch on the current device: 64-column slabs per gradient
 *             workgroup, u blocks, dQ blocks, dP blocks, 256-row chunks.  this_layer / prev as LOWRANK_COMBO takes them; both 0:
 *             the plan of LOWRANK_GRAD (nu = 0).  Returns -1 for a width the launchers refuse. */
enum pevit_lowrank_form {
    PEVIT_LOWRANK_U = 0, PEVIT_LOWRANK_GRAD = 1, PEVIT_LOWRANK_COMBO = 2, PEVIT_LOWRANK_U_F32 = 3, PEVIT_LOWRANK_GRAD_F32 = 4
};
typedef struct pevit_lowrank_args {
    const void* dqkv; const void* qT; const float* q32; float* u32; void* u_bf16_cols;
    const void* xn; const float* t; float* partial; float* dbias_partial;
    const void* xn_prev; const float* u32_prev; float* partial_prev;
    int32_t form, ld, ldx, chunks, B, H, N, E, xcd_order, this_layer, prev;
} pevit_lowrank_args;
typedef struct pevit_prep_lowrank_args {
    const float* rule1_l; const float* rule1_r; const float* rule2_l; const float* rule2_r; const float* q_left; const float* q_right;
    const float* a1q; const float* a2q; const float* a1v; const float* a2v;
    void* w_aug_rows; void* wT_aug_cols; float* q32; void* qT; void* q16;
    size_t arena_bytes, param_floats;
    int32_t method, layers, E, r, f32, ldw, ldwT;
    float ascale;
} pevit_prep_lowrank_args;
typedef struct pevit_chain_lowrank_args {
    const float* partial; const float* dbias_partial; float* G; float* rule_scratch; const float* params; float* grads;
    size_t partial_layer, dbias_layer, p_layer0, p_layer_stride;
    int32_t method, chunks, layers, E, r;
    float ascale;
} pevit_chain_lowrank_args;
int pevit_op_lowrank_ex(void* stream, const pevit_lowrank_args* args);
int pevit_op_prep_lowrank(void* stream, const pevit_prep_lowrank_args* args);
int pevit_op_chain_lowrank(void* stream, const pevit_chain_lowrank_args* args);
int pevit_op_rule_sum(void* stream, const float* rule_scratch, float* grads, int l_lo, int l_hi);
int pevit_op_lowrank_plan(int B, int N, int E, int this_layer, int prev, int32_t out[5]);
/* Test-only forms of the classifier head and of the small exact kernels around it (stem_head.hip, misc.hip, text.hip;
 * tests/test_gpu_head.py, tests/test_gpu_movers.py).  They add no kernel.
 *   pevit_op_head_ex: every member of the head launcher's parameter struct by name (zero-initialised = nothing set); all scratch is
 *             the caller's.  feat [B][D], W [C][D], bias [C] (or NULL), running_mean / running_var [D], ybn [B][D], rstd [D],
 *             logits [B][C], dlogits [B][C], dybn [B][D], loss [1], all f32.  labels [B] int64 -> cross entropy (ignore_index -100);
 *             targets [B][C] f32 -> BCE with logits; both NULL -> forward only (nothing behind logits is touched).  gW [C][D] and
 *             gb [C] ACCUMULATE (gW NULL: neither is written); dfeat [B][D] f32 (NULL: no backward through the BatchNorm, and
 *             dybn[0:B] keeps the cross-entropy row losses); dfeat_bf16 [B][D]: the bf16 copy of dfeat, or NULL.
 *             Refused here, before any launch: a NULL struct, B / D / C < 1, labels and targets both set, training with B < 2, a
 *             missing feat / W / running_mean / running_var / ybn / rstd / logits, a loss without dlogits / dybn / loss.
 *   the movers: the launchers' arguments as they stand (their own refusals apply).  f32 = 1: the bf16-declared output holds f32
 *             (the storage of the f32 verification mode).  pevit_op_im2col_ex: u8 = 1 -> uint8 pixels with mean3 / std3 (host
 *             pointers), u8 = 0 -> f32 pixels. */
typedef struct pevit_head_args {
    const float* feat; const int64_t* labels; const float* targets; const float* W; const float* bias; float* gW; float* gb;
    float* running_mean; float* running_var; float* ybn; float* rstd; float* logits; float* dlogits; float* dybn;
    float* loss; float* dfeat; void* dfeat_bf16;
    int32_t training, B, D, Cc;
} pevit_head_args;
int pevit_op_head_ex(void* stream, const pevit_head_args* args);
int pevit_op_conv_weight(void* stream, const float* w, void* out, int E, int K, int Kpad, int f32);
int pevit_op_cls_row(void* stream, const float* cls, const float* pos, float* x, int B, int N, int E);
int pevit_op_im2col_ex(void* stream, const void* images, int u8, const float* mean3, const float* std3, void* patches, int B, int R,
                       int P, int Kpad, int f32);
int pevit_op_cast_ex(void* stream, const float* src, void* dst, size_t n, float scale, int f32);
/* dst[c*ldd + r] = src[r*cols + c] * (r < scaled_rows ? scale : 1) */
int pevit_op_transpose(void* stream, const float* src, int rows, int cols, void* dst, int ldd, int scaled_rows, float scale, int f32);
/* to_internal: dst[(b*N+n)*E + e] = src[(n*B+b)*E + e]; else the inverse */
int pevit_op_permute_rows(void* stream, const float* src, float* dst, int N, int B, int E, int to_internal);
int pevit_op_zero(void* stream, void* ptr, size_t bytes);
int pevit_op_scale_f32(void* stream, float* p, size_t n, float scale);
/* x[s*N + n][:] = table[clamp(tokens[s][n], 0, V-1)][:] + pos[n][:] ; rows_out[s][:] = x[s*N + argmax_n tokens[s][n]][:] (first maximum) */
int pevit_op_text_embed(void* stream, const int64_t* tokens, const float* table, const float* pos, float* x, int S, int N, int E, int V);
int pevit_op_text_eot_gather(void* stream, const int64_t* tokens, const float* x, float* rows_out, int S, int N, int E);
/* measurement only: device buffer of 8 uint64 per workgroup that the next pevit_op_attn_fwd_delta launches fill with s_memtime
 * stamps at their phase boundaries (NULL switches it off).  The segmented launches (pevit_op_attn_fwd_delta_seg, every call on a
 * multi-slot context) take no stamps: they may have more workgroups than ceil(B H / 6). */
int pevit_debug_timeline(void* buf);
/* measurement only: `workgroups` 256-thread workgroups with `lds_bytes` of LDS each that keep their CU slots for `microseconds`
 * on `stream` -- what the kernels of an overlapped RCCL all-reduce do to the one-tile-per-CU GEMMs (scripts/r4_coresidency.py) */
int pevit_debug_occupy(void* stream, int workgroups, int lds_bytes, double microseconds);
int pevit_op_lowrank_u(void* stream, const void* dqkv, int ld, const void* qT, float* u32, void* u_cols, int B,
                       int H, int N, int E);
int pevit_op_lowrank_grad(void* stream, const void* xn, int ldx, const float* u32, const void* dqkv, int ld,
                          const float* t, float* partial, float* dbias_partial, int B, int H, int N, int E);
int pevit_op_lowrank_chunks(int T);
/* post-MLP bottleneck adapters (adapter_model.py:264-282, compacter_model.py:302-308,432-448), one layer:
 * G[e][j] = sum_r X[r][e] Y[r][j] as per-chunk partials [chunks][E][64] (+ column sums of X / Y, may be NULL) */
int pevit_op_tn_chunks(int T);
int pevit_op_tn_gemm64(void* stream, const void* X_bf16, int ldx, const void* Y_bf16, int ldy, float* partial, float* csx,
                       float* csy, int T, int E);
/* LayerNorm backward with trainable affine: dx = dres + LN'(dy); partial[blocks][3][E] = sums of dy*xhat, dy, dres */
int pevit_op_lna_blocks(int rows);
int pevit_op_ln_bwd_affine(void* stream, const float* dy, const float* x, const float* mean, const float* rstd,
                           const float* gamma, const float* dres, float* dx, void* dx_bf16, float* partial, int rows, int E);
/* out0[i] += sum_c partial[c][i]  (i < n), or with three outputs partial[c][3][n] -> out0/1/2; deterministic */
int pevit_op_colsum_reduce(void* stream, const float* partial, int chunks, int n, float* out0, float* out1, float* out2);
/* f32 master parameters -> bf16 panels wd [64][E], wdT [E][64], wu [E][64], wuT [64][E].  Adapter: p0 = down.weight
 * (64,E), p1 = up.weight (E,64).  Compacter: rule (4,4,4), p0..p3 = down.W_left, down.W_right, up.W_left, up.W_right */
int pevit_op_prep_bottleneck(void* stream, int method, const float* rule, const float* p0, const float* p1, const float* p2,
                             const float* p3, void* wd, void* wdT, void* wu, void* wuT, int E);
/* chain rule from the dense panel gradients Gd, Gu ([E][64] each) onto the reference's tensors inside `grads`
 * (accumulating) at float offsets off0.. (Adapter: down.weight, up.weight; Compacter: the four W_left / W_right) */
int pevit_op_chain_bottleneck(void* stream, int method, const float* Gd, const float* Gu, const float* rule,
                              const float* params, float* grads, int E, size_t off0, size_t off1, size_t off2, size_t off3);
/* images (B,3,R,R) f32 -> patches [B*(R/P)^2][Kpad] bf16, k = c*P*P + py*P + px, zero padded (conv1, model.py:1036) */
int pevit_op_im2col(void* stream, const float* images, void* patches_bf16, int B, int R, int P, int Kpad);
int pevit_op_im2col_u8(void* stream, const uint8_t* images, const float* mean3, const float* std3, void* patches_bf16, int B,
                       int R, int P, int Kpad);
/* knobs for A/B measurements, held in the context (ctx == NULL: the process-wide defaults that only the
 * context-free pevit_op_* entry points above use): "gemm_config" (-1 = per-problem heuristic, 0..5 = force a tile
 * configuration: 128x128, 64x128, 64x64 with 4 waves; 256x128, 256x256, 320x256 with 8 waves; 6 = 128x64 with 4 waves),
 * "gemm_persistent", "gemm_big" (0 = never pick the 8-wave tiles), "gemm_big_bias", "gemm_kswitch", "gemm_cfg_longk" /
 * "gemm_cfg_shortk" (configuration of the few-tile problems above / below kswitch), "gemm_ablate" (bit 0 skips the
 * k-loop, bit 1 the epilogue stores, bit 2 the operand stream, bit 3 ds_read + MFMA),
 * "gemm_streamk" (0 = never use the stream-K decomposition of the few-tile long-K products), "gemm_ksplit" (0 = never
 * use the one-tile-per-CU 160x128 / 96x128 k-split tile of the N = E products; 2 = also on problems of several rounds),
 * "gemm_ksplit_stagger" (2 = phased kernel, default; 1 / 0 = the alternate-k-tile kernel with / without the half-iteration
 * offset), "gemm_ksplit_small", "gemm_ksplit_mink", "gemm_kphase_nl" (requests in the LOAD section: 8, or between the
 * MFMAs: 2), "gemm_kz2" (1 = two workgroups per 160x128 tile, half of K each, where those tiles fill at most half the chip;
 * default 0: measured slower, profiles/r05_experiments.md), "gemm_stagger" (0 = legacy 8-wave kernel, 1 = staggered, 2 = also the 256x128 tile), "gemm_band",
 * "gemm_skinny" (0 = never use the few-row split-K kernel), "gemm_skinny_maxm" / "_mink" / "_slices", "gemm_sk_share" /
 * "gemm_sk_band" (with gemm_streamk = 2), "lowrank_xcd", "profile_all", "fused_attn_delta" (0 = delta_add + attn_fwd as two launches), "fp8_tail" (0 = t = xn P as a launch of its own with fp8 weights), "adapter_fused" (0 = the post-MLP adapter as separate
 * LayerNorm / GEMM launches), "lowrank_combo" (0 = lowrank_u and lowrank_grad as two launches per layer) and
 * "dx_stored" (ctx only).  A path knob takes effect at the next forward: a backward takes the paths of the forward whose
 * activations it uses;
 * returns 0, or -1 for an unknown key */
int pevit_tune(pevit_ctx* ctx, const char* key, int value);

/* Stream-K GEMMs hand partial tiles from workgroup to workgroup inside one launch; a consumer that waits ~1 s for a
 * partial gives up (the tile is then wrong) and raises an error word instead of hanging the GPU.  Synchronises the
 * stream, returns 1 if that ever happened on this context's workspace (ctx NULL: the workspace of the pevit_op_*
 * entry points) and clears the word, 0 otherwise, -1 on a HIP error.  The reference has no counterpart (its GEMMs are
 * ATen calls, model.py:675,817); the engine checks it after the first step. */
int pevit_streamk_error(pevit_ctx* ctx, void* stream);
/* The same word WITHOUT clearing it, and the number of optimizer updates pevit_sgd_step has withheld on device since the word
 * was raised (the fused SGD kernel leaves parameters and momentum untouched while it is non-zero, so a corrupted tile never
 * reaches them).  The word stays raised -- and every further update withheld -- until pevit_streamk_error clears it: a caller
 * that swallows the error cannot silently train on. */
int pevit_streamk_status(pevit_ctx* ctx, void* stream, unsigned* error_word, unsigned* skipped_updates);

/* ---- data-parallel gradient exchange without a collective-library kernel (the optional allreduce_flat) ----
 * The reference has no multi-process path at all (utils/comm.py:62-150 is dormant); `north_star` asks for an all-reduce of the flat
 * adapter-gradient buffer only.  One pevit_ar per process / GPU: a mailbox in device memory ([2][world][max_floats] + flags,
 * allocated by pevit_ar_create -- the only allocation), exported as an IPC handle (pevit_ar_handle_bytes() bytes, to be carried to
 * the peers by whatever the host has: torch.distributed object collectives, a file, MPI) and opened by every peer with
 * pevit_ar_import.  pevit_allreduce_flat then sums buf[0:n] over the ranks in place: one device-to-device copy of the
 * contribution into every peer's mailbox + one 4-byte flag copy behind it (copy engines over xGMI; no kernel on the sending GPU),
 * and a small local kernel that waits for the peers' flags and adds the contributions in RANK ORDER (identical bits on every
 * rank).  Asynchronous on `stream`; all calls of one pevit_ar must use the same stream, in the same order on every rank.
 * pevit_ar_error: 1 if a reduction ever gave up waiting for a peer (its buffer is then left unreduced); the word stays raised until
 * pevit_ar_reset (round 6: reading it no longer clears it). */
typedef struct pevit_ar pevit_ar;
int pevit_ar_create(pevit_ar** out, int rank, int world, size_t max_floats);
void pevit_ar_destroy(pevit_ar* ar);
int pevit_ar_handle_bytes(void);
int pevit_ar_export(pevit_ar* ar, void* handle_out);
int pevit_ar_import(pevit_ar* ar, int peer, const void* handle);
int pevit_allreduce_flat(pevit_ar* ar, void* stream, float* buf, size_t n);
int pevit_ar_error(pevit_ar* ar, void* stream);       /* 0 fine, 1 a peer never arrived, 2 the ranks passed different sizes */
/* Round 5.  The push is a kernel (stores through the IPC-mapped peer addresses, system-scope fence, one 8-byte release store per
 * peer flag); PEVIT_AR_PUSH=dma selects the copy-engine push of round 4, which an eight-process soak on one device showed to be
 * unreliable (torn / lost flags).  The flag a rank pushes is the pair (epoch, n); ONE workgroup of the reducing launch decides for all of them, so a bucket is
 * reduced everywhere or nowhere; the mailbox is fine-grained memory where the runtime exports such an allocation
 * (pevit_ar_fine_grained; PEVIT_AR_COARSE=1 forces the plain one).  pevit_ar_error_word: the device address of the error word, for
 * pevit_set_external_poison -- pevit_sgd_step then withholds the update of a step whose exchange failed (and writes NaN over that
 * step's loss), as it does for a stream-K hand-off error; the word stays raised until pevit_ar_reset clears it.
 * EXPERIMENTAL: exercised with 2 / 4 / 8 processes on ONE device only; the measured multi-GPU route is RCCL (torch.distributed). */
const unsigned* pevit_ar_error_word(pevit_ar* ar);
/* back to the initial protocol state (epoch 0, flags and error word cleared).  Collective by convention: every rank drains its device
 * and meets the others BEFORE and AFTER this call (dp.FlatAllReduce.resync does both). */
int pevit_ar_reset(pevit_ar* ar, void* stream);
int pevit_ar_fine_grained(pevit_ar* ar);
int pevit_set_external_poison(pevit_ctx* ctx, const unsigned* device_word);
/* Round 5 (data parallelism; no reference counterpart -- /root/reference/vision_benchmark/utils/comm.py is dormant): a hipEvent_t the
 * fused step (pevit_train_forward_backward[_u8]) waits for on its stream AFTER the stem (patch gather, patch embedding, class /
 * position rows, ln_pre: no trainable parameter, no gradient) and BEFORE the adapters are first read and the gradient buffer is
 * cleared.  Recorded by the caller behind the previous step's gradient exchange + pevit_sgd_step, which may then run on another
 * stream, under the next step's stem (engine.HipEngine dp_exchange_mode = "pipelined").  NULL detaches it. */
int pevit_set_step_gate(pevit_ctx* ctx, void* hip_event);

/* segmented predict on a multi-slot inference context: its four entry points */
#include "pevit_segments.h"
/* ... and the slot contexts of all four methods (Adapter and Compacter included): their two entry points */
#include "pevit_segments_all.h"
/* gradient-norm clipping over the flat gradient buffer, between the backward and the update: its three entry points */
#include "pevit_clip.h"

#ifdef __cplusplus
}
#endif
#endif /* PEVIT_HIP_H */
