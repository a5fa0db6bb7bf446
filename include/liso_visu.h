/*
 * liso_visu.h -- C ABI of the summary pictures on the device: the flow wheel, the top-down intensity image of a cloud, the
 * occupancy image of box centres, the bird's-eye corners of boxes as pixel indices, per-box colours from a colour table and the
 * anti-aliased lines that draw the boxes onto a canvas.  No host synchronisation (graph-capturable).
 *
 * Replaces, in liso/visu: flow_image.py:29-45 with color_conversion.py:5-21, pcl_image.py:46-157, and of bbox_image.py the
 * corners (:261-351), the two projections of draw_box_onto_image (:195-223), its colour forms (:233-252, :442-456) and
 * draw_line_on_image (:163-182) with skimage.draw.line_aa behind it.
 *
 * Conventions (as include/liso_label_prep.h): device pointers, caller-allocated outputs and workspaces, no allocation, no host
 * synchronisation; every entry point checks its arguments before it launches anything and returns LISO_OK, LISO_EINVAL,
 * LISO_EWORKSPACE or LISO_ELAUNCH.  Images are row-major.  The source file is compiled without FMA contraction: every expression
 * below is evaluated operation by operation, in the order written.
 */
#ifndef LISO_VISU_H
#define LISO_VISU_H

#include <stddef.h>
#include <stdint.h>

#include "liso_iou3d.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LISO_VISU_MAX_CELLS (1 << 24) /* h * w of one image */
#define LISO_VISU_MAX_N (1 << 24)     /* rows per cloud */
#define LISO_VISU_MAX_LINES 65535     /* lines per image in one call */
#define LISO_VISU_WALK_LINES 64       /* lines walked side by side, one lane each */

/* 1. Flow wheel.  flow fp32 [B, 2, h, w] -> rgb fp32 [B, 3, h, w], all in fp32:
 *     mag = sqrtf(fx*fx + fy*fy), max_mag = max of mag over the image, ang = atan2f(fy, fx),
 *     hue = (ang >= 0 ? ang : ang + 2pi) / 2pi, q = mag / max_mag, val = q < 1 ? q : 1     (a NaN q, from max_mag == 0, gives 1)
 *     h6 = hue * 6, x = val * (-(|fmodf(h6, 2) - 1|) + 1), sector = (int)h6 % 6,
 *     rgb = (val, x, 0), (x, val, 0), (0, val, x), (0, x, val), (x, 0, val), (val, 0, x) for sector 0..5.
 *   max_mag: fp32 [B] scratch.  Two launches. */
int liso_visu_flow_wheel_f32(int batch, int h, int w, const float* flow, float* max_mag, float* rgb, void* stream);

/* 2. Top-down image of padded clouds.  pcl fp32 [B, n_max, point_stride] (x, y first), intensity fp32 [B, n_max]; a row whose x or
 *   y is NaN is padding and takes no part.  Per cloud, lo / hi = the least / greatest non-NaN intensity of its rows; when lo < 0 or
 *   hi > 1 every intensity becomes (i - lo) / (hi - lo), else it stays.  With f = min(h / (max_x - min_x), w / (max_y - min_y)) in
 *   fp32, a row lies inside when min + 0.01f < p and p < max - 0.01f on both axes, and falls on pixel
 *   ((long)((x - min_x) * f), (long)((y - min_y) * f)) (truncation; a pixel outside the image is dropped).  Of the rows on one pixel
 *   the one with the highest index gives the value (a 64-bit atomicMax on (index + 1) << 32 | value bits).
 *   image fp32 [B, h, w] (0 where no row fell), occupied uint8 [B, h, w].  extent = {min_x, min_y, max_x, max_y}.
 *   workspace: liso_visu_topdown_workspace_bytes(batch, h, w) bytes, 256-byte aligned.  Three launches. */
size_t liso_visu_topdown_workspace_bytes(int batch, int h, int w);
int liso_visu_topdown_f32(int batch, int n_max, int point_stride, int h, int w, const float* pcl, const float* intensity,
                          const float* extent, float* image, uint8_t* occupied, void* workspace, size_t workspace_bytes,
                          void* stream);

/* 3. Occupancy image of points (box centres).  pts fp64 [B, n, pt_stride] (x, y first), valid uint8 [B, n] or NULL (every row):
 *   image fp32 [B, h, w] = 1 at (min(max(trunc(((x + 0.5*range_x) / range_x) * h), 0), h - 1), likewise y, range_y, w), else 0;
 *   fp64, truncation as numpy's astype(int32) (a NaN lands on 0).  Two launches (zero, mark). */
int liso_visu_occupancy_f64(int batch, int n, int pt_stride, int h, int w, double range_x, double range_y, const double* pts,
                            const uint8_t* valid, float* image, void* stream);

/* 4. Bird's-eye corners of boxes as pixel indices.  pos fp64 [B, S, 3], dims fp64 [B, S, 3], rot fp64 [B, S]; rowcol int32
 *   [B, S, 5, 2].  Every slot is computed, valid or not (the drawing skips invalid ones).  Corners in the box frame, in order:
 *   (+hx, +hy), (-hx, +hy), (-hx, -hy), (+hx, -hy) and the top hat (hx + hy, 0) with hx = 0.5*dx, hy = 0.5*dy.  With c = cos(rot),
 *   s = sin(rot) in fp64, the sensor point is ((c*lx + (-s)*ly) + tx, (s*lx + c*ly) + ty); with pose_f32 != 0 c, s, the box-frame
 *   corner and the position are rounded to fp32 first and the two expressions are evaluated in fp32.  The result is rounded to
 *   fp32 (p) and projected in fp32:
 *     range_form == 2: rint(((p + 0.5f*range) * grid) / range) per axis (half to even), range = extent[0..1], grid = (h, w);
 *     range_form == 4: (long)((p - min) * f) with min, f of entry 2, extent = {min_x, min_y, max_x, max_y}.
 *   A value that is NaN or outside int32 gives INT32_MIN.  dims_lo <= dims_hi clamp dx, dy first when dims_lo > 0 (0: no clamp).
 *   One launch. */
int liso_visu_box_corners_bev(int batch, int n_slots, int h, int w, int range_form, const float* extent, int pose_f32,
                              double dims_lo, double dims_hi, const double* pos, const double* dims, const double* rot,
                              int32_t* rowcol, void* stream);

/* 5. Per-box colours from a 256-entry table.  scalar fp32 [B, S], valid uint8 [B, S], table fp64 [256, 3]; colors fp64 [B, S, 3].
 *   Per image lo / hi = min / max of the scalar over the valid slots, and in fp32
 *     mode 0 (draw_box_onto_image's "confidence"): t = lo != hi ? (v - lo) / (hi - lo) : 1,
 *     mode 1 (attribute_colored_box_image):        t = (v - lo) / max(hi - lo, 1e-6f), and t = 0.5 in an image with no valid slot.
 *   colour = table[min(max((int)(t * 256), 0), 255)]; a NaN t gives (0, 0, 0).  Every slot gets a colour.  One launch. */
int liso_visu_box_colors(int batch, int n_slots, int mode, const float* scalar, const uint8_t* valid, const double* table,
                         double* colors, void* stream);

/* 6. Anti-aliased lines onto canvases, in place.  canvas fp32 [B, h, w, channels], channels 1, 3 or 4; endpoints int32
 *   [B, n_lines, 2, 2] = (row, col) of start and end; valid uint8 [B, n_lines / group] or NULL; colors fp64
 *   [B, n_lines / group, channels]: `group` consecutive lines (the five edges of a box) share one flag and one colour.
 *   With closed != 0 `endpoints` is int32 [B, n_lines, 2] instead, the corners of closed polygons of `group` corners each (entry
 *   4's table as it stands, group 5): line l runs from corner l to the next corner of its group, the last one back to the first.
 *   Lines apply in index order, each as
 *     canvas[r, c] = (float)((1 - wgt) * (double)canvas[r, c] + wgt * color)
 *   over the entries (r, c, wgt) of skimage.draw.line_aa(r0, c0, r1, c1) with r, c clipped to the canvas: every entry reads the
 *   canvas as it was before the line, and of the entries that clipping puts on one pixel the last in walk order is the one that
 *   counts.  The walk: dc = |c1 - c0|, dr = |r1 - r0|, err = dc - dr, ed = (double)(float)sqrt(dc*dc + dr*dr) (1 for a point);
 *   loop { emit (r, c, |err - dc + dr| / ed); e = err, c' = c;
 *          if (2e >= -dc) { if (c == c1) stop; if (e + dr < ed) emit (r + sr, c, |e + dr| / ed); err -= dr; c += sc; }
 *          if (2e <= dr)  { if (r == r1) stop; if (dc - e < ed) emit (r, c' + sc, |dc - e| / ed); err += dc; r += sr; } }
 *   and wgt = 1 - value, all in fp64.
 *   A valid line with an endpoint more than max_reach pixels outside the canvas on either axis (r < -max_reach,
 *   r > h - 1 + max_reach, likewise c; INT32_MIN from entry 4 always is) is not drawn; overflow[b] (int32 [B], optional) is
 *   increased by the number of such lines.  0 <= max_reach <= 1 << 20.
 *   workspace: liso_visu_lines_workspace_bytes(batch, h, w, max_reach) bytes, 256-byte aligned.  One launch, one workgroup per
 *   image. */
size_t liso_visu_lines_workspace_bytes(int batch, int h, int w, int max_reach);
int liso_visu_draw_lines_f32(int batch, int h, int w, int channels, int n_lines, int group, int closed, int max_reach,
                             const int32_t* endpoints, const uint8_t* valid, const double* colors, float* canvas, int32_t* overflow, void* workspace,
                             size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LISO_VISU_H */
