/* Segmented predict for all four methods: slot contexts for the post-MLP adapters (Adapter, Compacter) next to those of the
 * attention-site methods (pevit_segments.h).  Part of the C ABI of pevit_hip.h, which includes this file behind pevit_segments.h;
 * the rules of that header and the semantics of pevit_segments.h (segments, slots, pevit_predict_segments[_u8] and their refusals) hold.
 *
 * The post-MLP adapters are row-wise: a token row needs only its own segment's LayerNorm affine, down and up panels and biases, and
 * there is no raw reshape, so an image's answer depends on no other row.  A slot of such a context keeps, per layer, one [64][E] bf16
 * down panel and one [E][64] bf16 up panel resident in the arena; a segmented call runs the frozen products once on all rows and the
 * adapter per segment on its slot's panels: on the fused route ONE launch per layer whose workgroups never cross a segment end
 * (csrc/adapter_fused.hip adapter_fwd_seg_kernel), on the unfused route (widths that are no multiple of 256, or "adapter_fused" tuned
 * 0) LayerNorm, down and up product per segment on its row range.  The answer for a segment is what pevit_predict computes for that
 * segment's images alone with that slot's adapter, head and BatchNorm statistics.
 *
 * pevit_infer_create_slots_all: KAdaptation / LoRA: pevit_infer_create_slots itself -- same context, same sizes, same refusals.
 *   Adapter / Compacter in bf16 with 1 <= slots <= 8: the arena of pevit_infer_create plus, per layer and slot, the two panels
 *   (nothing else grows: the transposed stores of the panel kernels go to the context's write-only panel); the workspace is byte for
 *   byte that of pevit_infer_create.  slots == 1 gives the context of pevit_infer_create.  Refused by name with slots > 1: method
 *   none, the fp8 formats, the f32 verification mode; bad dims are refused in the words of pevit_infer_create.
 * pevit_load_adapter_slot_rule: pevit_load_adapter_slot with Compacter's frozen (4,4,4) rule as a device pointer.  The rule is read
 *   only while the panels are built and does not pass through the arena: the rule pevit_load_phm_rule gave the single-adapter calls
 *   stays as it is.  On an Adapter context phm_rule must be NULL (pevit_load_adapter_slot does the same there); on a Compacter slot
 *   context pevit_load_adapter_slot, which has no rule to give, is refused.  On the attention-site contexts phm_rule must be NULL too.
 *   The f32 vectors (LayerNorm affine, b_down, b_up) and the head are read from params by every later segmented call, so the buffer
 *   must stay alive while the slot is loaded; the f32 sources of the panels are not read again.
 * pevit_load_block empties every slot.  The single-adapter calls run on such a context with the bits of a pevit_infer_create
 * context, interleaved freely with segmented calls: their panels keep their own place.
 *
 * Out of scope: the fp8 formats and the f32 verification mode on slot contexts, pevit_encode_image / pevit_zeroshot by segments,
 * more than 8 slots or 16 segments, an inference form of the unsegmented fused kernel. */
#ifndef PEVIT_SEGMENTS_ALL_H
#define PEVIT_SEGMENTS_ALL_H

int pevit_infer_create_slots_all(const pevit_dims* dims, int slots, pevit_ctx** out);
int pevit_load_adapter_slot_rule(pevit_ctx* ctx, void* stream, int slot, const float* params, int num_classes, const float* phm_rule);

#endif /* PEVIT_SEGMENTS_ALL_H */
