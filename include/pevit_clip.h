/* Gradient-norm clipping inside the fused step.  Part of the C ABI of pevit_hip.h, which includes this file; the rules of that
 * header (one stream per context, device pointers, 0 = success, pevit_last_error) hold here.
 *
 * torch.nn.utils.clip_grad_norm_(parameters, max_norm) with norm_type = 2 and error_if_nonfinite = False, in f32, over the flat
 * gradient buffer, as two launches (csrc/clip.hip) with no host read in between:
 *     total = grad_scale * sqrt(sum g^2)         squares and the sums inside a workgroup in f32, the sum over the workgroups' partials
 *                                                in f64, every sum in one fixed order: the same buffer gives the same bits on every call
 *     coef  = min(1, max_norm / (total + 1e-6f))
 *     g    *= coef                               always multiplied, as torch does; coef == 1 changes no bit
 * A NaN anywhere makes total and coef NaN and with them every counted element; total = +inf gives coef = 0.  grad_scale is the
 * factor the update kernels take (1 / world under data parallelism, where the buffer holds the sum over the ranks): it scales the
 * NORM only -- the buffer is multiplied by coef alone and the update applies grad_scale as before.
 *
 * scratch: caller-owned device f32 words, pevit_clip_scratch_floats(n) of them, zeroed ONCE by the caller; a launch leaves the
 * words it counts arrivals in zero again.  After the launches scratch[0] = total (the norm BEFORE clipping) and scratch[1] = coef:
 * the host may read both behind the step, the engine never synchronises for them.  No workspace layout or size changes.
 *
 * pevit_clip_grad_norm: the context's gradient buffer (pevit_set_params' grads, pevit_num_params elements) under the device mask it
 * was given (pevit_param_grad_mask: KAdaptation's v_proj_adapter1_*, whose .grad is None in torch, are neither counted nor
 * touched).  Refused before any launch: a null context / scratch / gradient buffer (a context without parameters), an
 * inference-only or text context, max_norm or grad_scale that is not finite or not > 0.  The stream-K error word and the external
 * poison word do not gate it: they go on withholding the update behind it.
 * pevit_op_clip_grad_norm: the same two launches on any 16-byte aligned f32 buffer of n >= 1 elements, context-free (tests,
 * measurements); mask_or_null: one byte per element, 4-byte aligned, 0 = neither counted nor scaled. */
#ifndef PEVIT_CLIP_H
#define PEVIT_CLIP_H

size_t pevit_clip_scratch_floats(size_t n);
int pevit_clip_grad_norm(pevit_ctx* ctx, void* stream, float max_norm, float grad_scale, float* scratch);
int pevit_op_clip_grad_norm(void* stream, float* g, const unsigned char* mask_or_null, size_t n, float max_norm, float grad_scale,
                            float* scratch);

#endif /* PEVIT_CLIP_H */
