/* Segmented predict: requests for several adapters in one engine call.  Part of the C ABI of pevit_hip.h, which includes this file;
 * the rules of that header (one stream per context, device pointers, 0 = success, pevit_last_error) hold here.
 *
 * An inference-only context created here keeps up to 8 adapter SLOTS resident in its arena: per layer the 64 bf16 rows of P behind
 * the frozen in_proj rows, one slot after the other, and the bf16 panel of Q.  pevit_load_adapter_slot builds them once; a segmented
 * call builds nothing and reads them all in ONE walk: its QKV product has 3 width + 64 slots output columns, and the attention site
 * adds each segment's delta with that segment's slot.
 *
 * Semantics.  A segmented call takes B images split into nseg contiguous segments (first image, count, slot) that tile [0, B) in
 * order, one image at least each; two segments may name the same slot.  The answer for a segment is what pevit_predict computes for
 * that segment's images ALONE, as a batch of `count`, with that slot's adapter, head and BatchNorm statistics: the raw reshape of the
 * adapter delta (model.py:796-799), which makes an image's logits depend on its batch, works inside the segment.  A request's
 * answer therefore does not depend on who shares the launch with it.  Everything outside the attention site is row-wise and runs
 * once on all rows.
 *
 * All four methods are served by segments.  This header holds the entries of the attention-site methods and the two calls;
 * Adapter and Compacter, whose adapters are row-wise, get their slot contexts from pevit_infer_create_slots_all and their slots from
 * pevit_load_adapter_slot_rule (pevit_segments_all.h, included behind this file), and are answered by the same two calls below.
 *
 * pevit_infer_create_slots: pevit_infer_create with 1 <= slots <= 8 slots.  KAdaptation and LoRA in the bf16 weight format only: the
 * post-MLP methods (this entry keeps refusing them: their slots are another arena, see pevit_infer_create_slots_all), method none,
 * the fp8 formats and the f32 verification mode
 * are refused with slots > 1 (with slots == 1 they give the context of pevit_infer_create, which refuses the segmented calls).
 * pevit_infer_create itself is unchanged: same arena, same workspace.  The arena grows by 64 slots rows of in_proj and `slots` Q
 * panels per layer, the workspace by 64 slots f32 columns of t per token.
 * pevit_load_adapter_slot: params as pevit_set_infer_params takes them, 1 <= num_classes <= dims.num_classes.  Builds the slot's
 * panels on the stream (the one launch the per-call walk makes for the selected adapter) and remembers the pointer: the delta bias
 * (KAdaptation) and the head are read from it by every later segmented call, so the buffer must stay alive while the slot is loaded.
 * pevit_load_block empties every slot (it rewrites the rows they live behind).
 * pevit_predict_segments[_u8]: segs is a HOST array.  logits: dense (count x num_classes of the slot) f32 per segment; features:
 * (count x out_dim) f32 or NULL.  Refused before any launch: segments that do not tile [0, B), a slot outside the context or not
 * loaded, B outside [1, max_batch], nseg outside [1, 16], a null pointer, a context of pevit_infer_create.
 * The single-adapter calls (pevit_set_infer_params, pevit_predict, pevit_encode_image, pevit_zeroshot and their _u8 forms) run on such
 * a context too, interleaved freely with segmented calls: their per-call panels live in a place of their own behind the slots, so
 * neither kind disturbs the other, and their results are the bits of the same call on a pevit_infer_create context. */
#ifndef PEVIT_SEGMENTS_H
#define PEVIT_SEGMENTS_H

#define PEVIT_MAX_SLOTS 8
#define PEVIT_MAX_SEGMENTS_PER_CALL 16

typedef struct pevit_segment {
    int32_t first, count, slot;
    const float* running_mean;      /* (out_dim) eval-mode BatchNorm statistics of the segment's head */
    const float* running_var;
    float* logits;                  /* (count x num_classes of the slot) */
    float* features;                /* (count x out_dim), or NULL */
} pevit_segment;

int pevit_infer_create_slots(const pevit_dims* dims, int slots, pevit_ctx** out);
int pevit_load_adapter_slot(pevit_ctx* ctx, void* stream, int slot, const float* params, int num_classes);
int pevit_predict_segments(pevit_ctx* ctx, void* stream, const float* images, int batch, int nseg, const pevit_segment* segs);
int pevit_predict_segments_u8(pevit_ctx* ctx, void* stream, const uint8_t* images, int batch, int nseg, const pevit_segment* segs);

#endif /* PEVIT_SEGMENTS_H */
