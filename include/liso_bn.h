/*
 * liso_bn.h -- C ABI of the fused BatchNorm2d(+ReLU) for channels-last BEV feature maps (gfx950).
 *
 * Replaces the norm + activation pairs of the reference's BEV backbone / head
 *   liso/networks/centerpoint/rpn.py:113-131 (`BatchNorm2d` + `ReLU` after every conv; built by norm.py:55-56)
 *   liso/networks/centerpoint/center_head.py:36-38,81-92
 * which PyTorch runs as 3 (forward) + 3 (backward) BatchNorm launches plus separate ReLU kernels.  Here:
 *   forward  = stats (1 read of x) -> finalize (tiny) -> apply+ReLU (1 read, 1 write)
 *   backward = reduce (read dy, x) -> finalize (tiny) -> dx (read dy, x; write dx), ReLU mask recomputed from x
 * Batch statistics use block-shifted sums merged over the block means in fp64 (fixed order):
 * no E[x^2]-E[x]^2 cancellation (MIOpen's spatial BN loses ~2e-4 relative at mean/std = 50, measured), reproducible.
 *
 * x, y, dy, dx: [M, C] row-major (M = N*H*W pixels, channels-last), dtype by element code (include/liso_conv.h): fp32 (is_bf16 = 0),
 * bf16 (is_bf16 = 1) or fp16 (is_bf16 = 2; the BatchNorm entry points only -- the InstanceNorm ones return LISO_EINVAL for it);
 * C % 8 == 0, C <= 256 (V = 4 channels per lane in fp32, 8 in bf16 / fp16; 256 / (C / V) rows per block pass).  gamma/beta/running_*: fp32 [C].  stats: fp32 [4*C] = scale | shift | mean | invstd.
 * All pointers are device pointers; nothing allocates or synchronises.
 */
#ifndef LISO_BN_H
#define LISO_BN_H

#include <stddef.h>
#include <stdint.h>

#include "liso_conv.h" /* liso_wgrad_reduce_job */

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of device scratch for the calls below (depends only on C) */
size_t liso_bn_workspace_bytes(int c);

/* training != 0: batch statistics (biased variance for normalisation, unbiased for running_var, torch semantics),
 * running stats updated in place with `momentum`;  training == 0: running statistics.  relu != 0 fuses max(.,0). */
int liso_bn_relu_fwd(const void* x, int is_bf16, long m, int c, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, float momentum, float eps, int training, int relu,
                     void* y, float* stats, void* workspace, size_t workspace_bytes, void* stream);

/* grad_gamma/grad_beta [C] fp32 overwritten; dx has the dtype of x. */
int liso_bn_relu_bwd(const void* dy, const void* x, int is_bf16, long m, int c, const float* gamma, const float* stats,
                     int training, int relu, void* dx, float* grad_gamma, float* grad_beta, void* workspace,
                     size_t workspace_bytes, void* stream);

/* The same backward on rows that are CHANNEL SLICES of wider channels-last tensors: row r of dy / x / dx starts dy_stride / x_stride /
 * dx_stride elements after row r - 1 (>= C, multiples of 16 bytes; the pointers address the slice's first channel).  The BatchNorms
 * behind a channel concatenation (the three deblocks in front of the head, liso/networks/centerpoint/rpn.py:140-146) then read and
 * write the concatenated tensors in place: no slice copies, no concatenation of the partial input gradients. */
int liso_bn_relu_bwd_strided(const void* dy, long dy_stride, const void* x, long x_stride, int is_bf16, long m, int c, const float* gamma,
                             const float* stats, int training, int relu, void* dx, long dx_stride, float* grad_gamma, float* grad_beta,
                             void* workspace, size_t workspace_bytes, void* stream);

/* The superset of the two entries above, and the one the Python side calls: the three strides are all zero (dense rows, liso_bn_relu_bwd)
 * or all non-zero (liso_bn_relu_bwd_strided), and with job != NULL the finalize launch also carries the blocks of a deferred
 * weight-gradient slab reduction (include/liso_conv.h: liso_conv_wgrad_deferred): grid = the finalize's blocks first, then the
 * reduction's.  The two roles share the launch and nothing else -- no flag, fence or atomic between them; every block runs the
 * instructions of the separate launches on the same data, so all results are the same bits.  The finalize (latency-bound, a few blocks)
 * runs in the shadow of the reduction (bandwidth-bound), one launch less on the backward pass's dependent chain per layer.
 * job == NULL: exactly liso_bn_relu_bwd(_strided). */
int liso_bn_relu_bwd_chained(const void* dy, long dy_stride, const void* x, long x_stride, int is_bf16, long m, int c, const float* gamma,
                             const float* stats, int training, int relu, void* dx, long dx_stride, float* grad_gamma, float* grad_beta,
                             void* workspace, size_t workspace_bytes, const liso_wgrad_reduce_job* job, void* stream);

/* ---- grouped backward with one or two upstream gradients --------------------------------------------------------------------
 * One raw channels-last tensor x (rows of x_stride elements) carries up to LISO_BN_MAX_GROUPS BatchNorms over ascending, disjoint
 * channel ranges [c_off, c_off + c), c <= 256, c_off on a 16-byte boundary (the deblocks' 3 x 128-channel concatenation), and receives
 * one or two gradients dy_a / dy_b (dy_b == NULL: one) -- a map with two consumers, each handing back dL/d(relu(bn(x))) for its own
 * use of it.  x, dy_a, dy_b and dx address channel 0 of their rows, each with its own row stride.  The call is three launches:
 *   reduce    grid (row blocks, groups): per (group, gradient) the device function that is liso_bn_relu_bwd_strided's reduce pass, on
 *             that group's channels alone (its geometry, row order and LDS summation order) -> the same partial sums, bit for bit; x
 *             and the ReLU mask are read once per row for both gradients.
 *   finalize  one block per channel segment of every group (the segments and merge order of the single call), both gradients in turn;
 *             the parameter gradients written are fl(fl(sum_a) + fl(sum_b)) -- what adding the second single call's result onto the
 *             first one's gives in fp32 -- and the dx coefficients stay per gradient.  Behind these blocks ride the slab reductions of
 *             up to two deferred weight gradients (job_a / job_b, NULL: none), as in liso_bn_relu_bwd_chained.
 *   dx        per element dx_a and dx_b by the single calls' own dx device function, each rounded to the element type, then
 *             round(float(dx_a) + float(dx_b)): the elementwise sum of the two stored maps.  One gradient: dx_a.
 * No atomics, no flags between blocks; every group's grad_gamma / grad_beta [c] fp32 are overwritten.  `training` / `relu` hold for
 * all groups of the call. */
#define LISO_BN_MAX_GROUPS 4
typedef struct liso_bn_group {
    int c_off, c;
    const float* gamma;
    const float* stats; /* [4 * c] = scale | shift | mean | invstd of this group */
    float* grad_gamma;
    float* grad_beta;
} liso_bn_group;
size_t liso_bn_multi_workspace_bytes(const liso_bn_group* groups, int n_groups, int n_grads);
int liso_bn_relu_bwd_multi(const void* dy_a, long dy_a_stride, const void* dy_b, long dy_b_stride, const void* x, long x_stride, int elem,
                           long m, const liso_bn_group* groups, int n_groups, int training, int relu, void* dx, long dx_stride,
                           void* workspace, size_t workspace_bytes, const liso_wgrad_reduce_job* job_a, const liso_wgrad_reduce_job* job_b,
                           void* stream);
/* host only: LISO_OK where liso_bn_relu_bwd_multi accepts this table and these strides (-> the finalize launch's segment blocks),
 * LISO_EINVAL otherwise (more than 4 groups, a group wider than 256 channels, overlapping or unaligned ranges, a range past a row) */
int liso_bn_relu_bwd_multi_check(const liso_bn_group* groups, int n_groups, int n_grads, int elem, long m, long x_stride,
                                 long dy_a_stride, long dy_b_stride, long dx_stride, int* n_finalize_blocks);

/* ---- InstanceNorm2d(+ReLU), training: the same passes with one set of statistics per sample ---------------------------------
 * Replaces `nn.InstanceNorm2d(affine=True)` + `ReLU` of the SLIM encoders in training (liso/slim/model/extractor.py:24-38,
 * 219-230; norm_fn "instance" / "instance_affine"), which PyTorch runs through the BatchNorm kernels on a [1, B*C, H, W] view
 * (weight / bias repeated B times) in NCHW.  x, y, dy, dx: [groups, m, C] channels-last (groups = samples, m = H*W pixels each);
 * stats fp32 [groups, 4*C]; grad_gamma / grad_beta fp32 [groups, C] (per sample: the caller adds the samples).
 * No running statistics (track_running_stats = False). */
size_t liso_in_workspace_bytes(int groups, int c);
int liso_in_relu_fwd(const void* x, int is_bf16, int groups, long m, int c, const float* gamma, const float* beta, float eps, int relu,
                     void* y, float* stats, void* workspace, size_t workspace_bytes, void* stream);
int liso_in_relu_bwd(const void* dy, const void* x, int is_bf16, int groups, long m, int c, const float* gamma, const float* stats,
                     int relu, void* dx, float* grad_gamma, float* grad_beta, void* workspace, size_t workspace_bytes, void* stream);
/* The same backward with grad_gamma / grad_beta fp32 [C] = the SUM over the samples (what the shared affine parameters receive),
 * added in sample order inside the finalize launch: no [groups, C] intermediate, no reduction launches behind the call. */
int liso_in_relu_bwd_sum(const void* dy, const void* x, int is_bf16, int groups, long m, int c, const float* gamma, const float* stats,
                         int relu, void* dx, float* grad_gamma, float* grad_beta, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LISO_BN_H */
