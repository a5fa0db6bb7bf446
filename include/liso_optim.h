/*
 * liso_optim.h -- C ABI of the detector's parameter update (gfx950): decoupled-weight-decay Adam over ONE flat fp32 buffer.
 *
 * Replaces torch.optim.AdamW.step() as the reference calls it in the detector train step
 *   liso/liso_cli.py:615-618   loss.backward(); optimizer.step(); lr_scheduler.step()
 *   liso/liso_cli.py:792-823   AdamW(box_predictor.parameters(), lr, weight_decay=0.01) driven by OneCycleLR (which rewrites
 *                              lr AND beta1 of the parameter group before every step)
 * which PyTorch runs as ~12 multi-tensor launches over ~100 parameter tensors (1.2 ms of host time per step on this path,
 * measured).  Here parameters, gradients and both moments live in four flat buffers with identical element order (the
 * trainer makes every nn.Parameter / .grad a strided view into them): the update is one HBM-bound pass,
 * 16 B read + 12 B written per element.
 *
 * Arithmetic per element (fp32, the operation order of torch/optim/adamw.py `_multi_tensor_adamw`, maximize = amsgrad = 0):
 *   p   <- p * (1 - lr * weight_decay)
 *   m   <- m + (1 - beta1) * (g - m)
 *   v   <- v * beta2 + (1 - beta2) * g * g
 *   p   <- p - (lr / (1 - beta1^step)) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * `step` is the 1-based count of THIS update.  The scalar factors are evaluated in double on the host side of the call.
 * All pointers are device pointers; nothing allocates or synchronises; the call enqueues on `stream` and returns LISO_OK or
 * a negative LISO_E* code (include/liso_iou3d.h).  Graph-capturable (the scalars are then baked into the captured node).
 */
#ifndef LISO_OPTIM_H
#define LISO_OPTIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int liso_adamw_step_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1,
                        double beta2, double eps, double weight_decay, long step, void* stream);

/* The same update on grad * grad_scale: data-parallel training all-reduces the flat gradient buffer with SUM and passes
 * grad_scale = 1 / world_size here instead of launching a division over the buffer (the reference is single-GPU; the gradient mean
 * over ranks is this build's addition).  grad_scale = 1 is bit-identical to liso_adamw_step_f32. */
int liso_adamw_step_scaled_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1,
                               double beta2, double eps, double weight_decay, double grad_scale, long step, void* stream);

/* liso_adamw_step_packed_f32, further down: the same update, whose launch also writes the convolutions' packed filter panels. */

/* ---- dynamic loss scaling (fp16 training) ---------------------------------------------------------------------------------------
 * The state lives in device memory and never travels to the host inside a step: the backward pass is seeded with `scale` (read from
 * device memory, so a captured hipGraph replays with the current value), then
 *   (a) liso_grad_nonfinite_f32     one pass over the flat fp32 gradient buffer: sets found_inf = 1 if any element is inf / NaN;
 *   (b) liso_adamw_step_amp_f32     the AdamW update above on grad * grad_scale / scale at bias-correction step `step + 1` -- or, with
 *                                   found_inf set, nothing at all (param, exp_avg, exp_avg_sq and `step` keep their bits);
 *   (c) liso_loss_scale_update      torch.cuda.amp.GradScaler.update() semantics: found_inf -> scale *= backoff_factor, growth_tracker
 *                                   = 0, skipped += 1; else step += 1 and growth_tracker += 1, reaching growth_interval -> scale *=
 *                                   growth_factor (if the product is finite), growth_tracker = 0.  Clears found_inf for the next step.
 * `step` advances on applied updates only, as torch.optim.AdamW's under GradScaler (its optimizer.step() is not called on a skipped
 * step).  A fixed loss scale is growth_factor = backoff_factor = 1: overflowing steps are still skipped.
 * Several ranks need nothing extra: the flat buffer is SUM-all-reduced before (a), so an inf / NaN on any rank is one on every rank, and
 * every rank takes the same decision on identical states.
 * One state per optimizer; the calls of one step are enqueued on one stream in the order (a), (b), (c).  Zero-initialised state with
 * `scale` set is a valid start.  The state is a device pointer aligned to 16 bytes, like the flat buffers (every call returns LISO_EINVAL
 * otherwise); the gradient / parameter / moment buffers of (a) and (b) are 16-byte aligned as for liso_adamw_step_f32. */
typedef struct {
    float scale;        /* the current loss scale */
    int found_inf;      /* set by (a), consumed and cleared by (c) */
    int growth_tracker; /* consecutive applied steps since the scale last changed */
    int step;           /* applied AdamW updates (bias-correction counter) */
    int skipped;        /* skipped steps (diagnostics) */
    int reserved[3];
} liso_loss_scale_state;

int liso_grad_nonfinite_f32(const float* grad, size_t n, liso_loss_scale_state* state, void* stream);
int liso_adamw_step_amp_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1,
                            double beta2, double eps, double weight_decay, double grad_scale, const liso_loss_scale_state* state,
                            void* stream);
int liso_loss_scale_update(liso_loss_scale_state* state, double growth_factor, double backoff_factor, int growth_interval, void* stream);

/* ---- the update that also writes what is derived from the parameters ------------------------------------------------------------------
 * Between the update and the next step's first convolution a training step used to rebuild, from the fp32 master weights, the packed
 * filter panels of every convolution (include/liso_conv.h: "Packed weights") and the merged filters of convolutions that run as one
 * launch (concatenated / block-diagonal filters and their biases).  None of that is arithmetic the result needs: the weights are in
 * registers once per step, inside the update.  liso_adamw_step_packed_f32 is liso_adamw_step_scaled_f32 -- every element of the flat
 * buffers is updated exactly once by the same device function, bit for bit -- whose launch also writes, for each listed tensor
 * [d0][d1][kh][kw] of the flat buffers:
 *   - up to two panel destinations (forward / data gradient), with the geometry and the bytes of liso_conv_pack_weights(_placed): mode
 *     LISO_CONV_BF16, LISO_CONV_F32X3 (hi / lo planes) or LISO_CONV_F32, the tensor placed at (k_offset, n_offset) of a panel whose K / N
 *     may be larger than the tensor's -- so one filter fills its range of a merged convolution's panel or its diagonal block of a
 *     block-diagonal one;
 *   - one "mirror": the updated fp32 values stored a second time as d0 rows of d1 * kh * kw floats, `mirror_row_stride` floats apart
 *     (the merged fp32 filter tensors and concatenated biases; a bias is d0 = 1, d1 = its length).
 * Only chunks that hold values of a tensor are written: padding (k >= K, n >= N, off-diagonal blocks) is zero-filled once, when the
 * panels are allocated (liso_conv_pack_weights_placed with clear = 1, which is also the repack whenever the parameters were changed by
 * anything but this call).
 * The table is checked and laid out on the host, once: liso_adamw_pack_table_plan -> its size and the launch's block count;
 * liso_adamw_pack_table_fill -> the image, which the caller copies to device memory (16-byte aligned) and passes to every step.
 * LISO_EINVAL (nothing is written or launched): a null or misaligned pointer (panels 16 bytes, mirrors 4), a tensor beyond `n`, not at
 * a multiple of 4 elements or overlapping another, a placement beyond its panel, two destinations sharing a 16-byte chunk, panels /
 * mirrors that overlap, a mode other than the three above, more than 64 taps.  Work items are 256-thread blocks: tiles of the listed
 * tensors (the new values pass through <= 16.3 KiB of LDS on their way into the panels) and float4 ranges of everything else. */
typedef struct {
    void* dst;              /* the panel (liso_conv_packed_bytes(K, N, kh * kw, mode) bytes) */
    int for_dgrad, mode;    /* as liso_conv_pack_weights, with the item's `transposed` */
    int K, N;               /* the panel's channel counts */
    int k_offset, n_offset; /* where the tensor's (0, 0) lands */
} liso_adamw_pack_dest;
typedef struct {
    size_t offset;          /* first element in the flat buffers */
    int d0, d1, kh, kw, transposed;
    int n_dest;             /* 0 .. 2 */
    liso_adamw_pack_dest dest[2];
    float* mirror;          /* NULL: none */
    size_t mirror_row_stride;
} liso_adamw_pack_item;
int liso_adamw_pack_table_plan(const liso_adamw_pack_item* items, int n_items, size_t n, size_t* bytes, int* blocks);
int liso_adamw_pack_table_fill(const liso_adamw_pack_item* items, int n_items, size_t n, void* image, size_t bytes);
int liso_adamw_step_packed_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1,
                               double beta2, double eps, double weight_decay, double grad_scale, long step, const void* table,
                               int blocks, void* stream);

/* RMSprop over one flat fp32 buffer (SLIM's optimizer, liso/slim/experiment.py:200-219: torch.optim.RMSprop(lr) with its defaults
 * alpha 0.99, eps 1e-8, no momentum, not centered), the element-wise operations of torch's multi-tensor implementation:
 *     square_avg = square_avg * alpha + (1 - alpha) * g * g;   param = param - lr * g / (sqrt(square_avg) + eps),   g = grad * grad_scale
 * All buffers 16-byte aligned; one launch. */
int liso_rmsprop_step_f32(float* param, const float* grad, float* square_avg, size_t n, double lr, double alpha, double eps,
                          double grad_scale, void* stream);

/* `count` fp32 arrays copied into their destinations by ONE launch per LISO_GATHER_MAX jobs: dst[k][0 .. numel[k]) = src[k][...].
 * The detector step uses it for the parameter gradients that autograd hands back as tensors of their own (merged / sliced
 * parameters whose gradient no kernel can write in place): with `.grad = None` autograd keeps those tensors instead of launching one
 * `add_` per parameter into the zeroed flat buffer (torch/csrc/autograd/functions/accumulate_grad.h), and this call moves all of
 * them into their flat-buffer slices.  src / dst / numel are HOST arrays of device pointers / element counts (baked into the launch). */
#define LISO_GATHER_MAX 48
int liso_gather_f32(int count, const void* const* src, void* const* dst, const size_t* numel, void* stream);

/* `n` device-to-device copies of any type in ONE launch per LISO_MULTI_COPY_MAX segments: dst[k][0 .. bytes[k]) = src[k][...]
 * (16-byte vectors where both pointers allow).  dst / src / bytes are HOST arrays (baked into the launch); segments must not overlap.
 * The training steps stage the inputs of their captured hipGraphs with it (10 target tensors per detector step, the cloud tensors of a
 * SLIM inference replay): one launch instead of one runtime buffer copy per tensor. */
#define LISO_MULTI_COPY_MAX 24
int liso_multi_copy(int n, void* const* dst, const void* const* src, const size_t* bytes, void* stream);

/* `n` 2-D copies in one launch per LISO_MULTI_COPY_ROWS_MAX jobs: job k copies rows[k] rows of row_bytes[k] contiguous bytes,
 * dst_stride[k] / src_stride[k] bytes between consecutive rows (everything a multiple of 4).  The merged filters of parallel
 * convolutions (block-diagonal / concatenated / channel-permuted: liso/slim/model/update.py:29-164 and
 * liso/networks/centerpoint/center_head.py:60-117 run their parallel branches as single launches) are assembled from the modules' own
 * parameters -- and their gradients handed back -- by one such launch instead of one framework copy per block. */
#define LISO_MULTI_COPY_ROWS_MAX 32
int liso_multi_copy_rows(int n, void* const* dst, const void* const* src, const unsigned* rows, const unsigned* row_bytes,
                         const size_t* dst_stride, const size_t* src_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LISO_OPTIM_H */
