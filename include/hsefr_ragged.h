/*
 * hsefr_ragged.h -- C ABI of libhsefr_ragged.so: one MTCNN detector pass over frames of DIFFERENT sizes
 * (hse_facerec_tf_amd/mtcnn.py, MTCNNDetector.detect_ragged; the reference's mtcnn_detect_faces, facial_analysis.py:478-604, which
 * takes one frame per call).
 *
 * hsefr.h's *_batch entries share a launch sequence among frames of one size: a frame is a grid index and two scalars (h, w) serve
 * all.  Here a pass is ONE list of (frame, pyramid level) items, each with its own dimensions and offsets in packed buffers, and one
 * launch per P-Net layer covers the whole list, whatever the number of levels:
 *   hsefr_ragged_pyramid       every level of every frame            (hsefr_mtcnn_pyramid_level per item)
 *   hsefr_ragged_conv2d        a P-Net convolution over all items    (hsefr_conv2d_direct per item)
 *   hsefr_ragged_maxpool       P-Net's pooling over all items        (hsefr_maxpool_f32 per item)
 *   hsefr_ragged_stage1        candidates, NMS, boxes, crop windows  (hsefr_mtcnn_stage1_level per item + _stage1_finish per frame)
 *   hsefr_ragged_crops         the R-Net / O-Net crops of all frames (hsefr_mtcnn_crops_batch with per-frame sizes)
 *   hsefr_ragged_stage_finish  stage 2 / 3 of all frames             (hsefr_mtcnn_stage_finish_batch with per-frame sizes)
 * The softmax (hsefr_softmax, row-wise on the packed [cells, 2] buffer) and R-Net / O-Net (hsefr_conv2d_direct on the crop lists)
 * need nothing new.  Every value is BIT FOR BIT what the entry in brackets gives for that item or frame: the one-frame bodies are the
 * same code (csrc/mtcnn_post_frame.h, csrc/area_resize_px.h, compiled into both libraries), and the convolution runs each output's
 * FMA chain in hsefr_conv2d_direct's order.
 *
 * Mapping threads to items: an item's thread range is padded to whole workgroups of 256 threads; the caller's plan gives every item
 * its first workgroup (`first_block`) and a workgroup -> item table (`d_block_item` [n_blocks]), so a workgroup looks its item up
 * once.  mtcnn.ragged_plan builds all tables on the host.
 *
 * The tables are the caller's and live on the device, so the library cannot check them before the launch.  The kernels check what
 * they read instead: an item, a frame or a range that does not lie inside the counts and buffer sizes passed next to the tables is
 * skipped (nothing read, nothing written), never followed out of bounds.
 *
 * A library of its own, as the album, frames and forest libraries are: libhsefr.so stays as it is (its size is bounded by its tests)
 * and they share no symbol -- this one has its own version number and its own per-thread error string.
 *
 * Conventions: those of hsefr.h -- extern "C", plain C types, 0 on success or a negative status (the values of hsefr_status), never
 * throws, data pointers are DEVICE pointers owned by the caller, launches are asynchronous on `stream` (a hipStream_t passed as
 * void*; NULL = the default stream).  Every scalar argument is checked before any device work; a call with nothing to do (zero items,
 * zero frames, zero crops) returns 0 without a launch, whatever the pointers; otherwise a null pointer is HSEFR_RAGGED_ERR_INVALID.
 * Built for gfx950 only.
 */
#ifndef HSEFR_RAGGED_H
#define HSEFR_RAGGED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSEFR_RAGGED_VERSION 100

#define HSEFR_RAGGED_OK 0
#define HSEFR_RAGGED_ERR_INVALID (-1)     /* bad argument                              */
#define HSEFR_RAGGED_ERR_UNSUPPORTED (-2) /* a case the kernels do not cover           */
#define HSEFR_RAGGED_ERR_HIP (-3)         /* a HIP runtime call failed                 */

/* a frame of the pass: uint8 RGB [h, w, 3] at byte `offset` of the packed frame buffer (ANY offset: frames stand back to back, so
 * an odd h * w * 3 puts the next frame on an odd address), and its items [first_item, first_item + n_items) in level order */
typedef struct {
    int64_t offset;
    int32_t h, w;
    int32_t first_item, n_items;
} hsefr_ragged_frame;                     /* 24 bytes */

/* a (frame, pyramid level) item of hsefr_ragged_pyramid: the level is float32 [dw, dh, 3] at ELEMENT offset level_off of the level
 * buffer.  rows != 0: one workgroup per destination row (the row form of hsefr_mtcnn_pyramid_level, with `hoff` its LDS split);
 * rows == 0: one thread per destination pixel.  Both forms give the same bits. */
typedef struct {
    int32_t frame, dh, dw, rows;
    int64_t level_off;
    int32_t first_block, hoff;
} hsefr_ragged_level;                     /* 32 bytes */

/* an item of one P-Net layer: the input map [ih, iw, c] at PIXEL offset in_off of x (element offset in_off * c), the output map
 * [oh, ow, cout] at pixel offset out_off of y */
typedef struct {
    int64_t in_off, out_off;
    int32_t ih, iw, oh, ow;
    int32_t first_block, reserved;
} hsefr_ragged_map;                       /* 40 bytes */

/* an item of hsefr_ragged_stage1: P-Net's output maps of one level, prob [w, h, 2] and reg [w, h, 4] at cell offset cell_off of the
 * packed buffers, and the level's scale */
typedef struct {
    int64_t cell_off;
    double scale;
    int32_t w, h;
} hsefr_ragged_cells;                     /* 24 bytes */

int hsefr_ragged_version(void);

/* the last failure on the calling thread ("" before the first) */
const char* hsefr_ragged_last_error_string(void);

/* rows of a candidate list (hsefr_mtcnn_post_capacity() of libhsefr.so: the same constant of the shared header) */
int hsefr_ragged_capacity(void);

/*
 * Every pyramid level of every frame in one launch: item i -> d_levels + d_items[i].level_off, float32 [dw, dh, 3], normalised and
 * transposed, the bits of hsefr_mtcnn_pyramid_level(frame, ., h, w, dh, dw).
 *   d_frames      uint8, frames_bytes bytes: the frames packed at d_frame_tab[f].offset
 *   d_frame_tab   [n_frames], d_items [n_items], d_block_item int32 [n_blocks]: item of every workgroup
 *   levels_elems  floats in d_levels;  lds_bytes  dynamic LDS of the launch: the largest need of an item with rows != 0 (0 .. 65536)
 * n_items == 0 or n_blocks == 0: returns 0, no launch.
 */
int hsefr_ragged_pyramid(const uint8_t* d_frames, int64_t frames_bytes, const hsefr_ragged_frame* d_frame_tab, int n_frames,
                         const hsefr_ragged_level* d_items, int n_items, const int32_t* d_block_item, int n_blocks, float* d_levels,
                         int64_t levels_elems, int lds_bytes, void* stream);

/*
 * y = PReLU(conv(x, w) + bias) over the item list in one launch: stride 1, VALID (pad_t == pad_l == 0; anything else is
 * HSEFR_RAGGED_ERR_UNSUPPORTED), w float32 [kh, kw, c, cout], bias / alpha [cout] or NULL.  A thread owns `co` (4, 2 or 1: cout a
 * multiple of it, w aligned to 4 * co bytes) consecutive output channels of one output pixel of one item, so an item has
 * oh * ow * (cout / co) threads, padded to whole workgroups by the plan.  Each output's FMA chain runs kh, kw, c ascending from the
 * bias: the bits of hsefr_conv2d_direct on that item, whatever co.
 *   x_pixels / y_pixels   pixels (of c / cout floats) in x / y: an item outside them, or with oh > ih - kh + 1 or ow > iw - kw + 1, is
 *                         skipped
 */
int hsefr_ragged_conv2d(const float* x, int64_t x_pixels, const float* w, const float* bias, const float* alpha, float* y, int64_t y_pixels,
                        const hsefr_ragged_map* d_maps, int n_items, const int32_t* d_block_item, int n_blocks, int c, int cout, int kh,
                        int kw, int stride, int pad_t, int pad_l, int co, void* stream);

/*
 * Max pooling k x k / stride with TensorFlow's SAME padding over the item list in one launch: windows clipped to the item, the bits
 * of hsefr_maxpool_f32.  oh == ceil(ih / stride), ow == ceil(iw / stride) (other items are skipped); a thread owns one channel of one
 * output pixel: oh * ow * c threads per item.
 */
int hsefr_ragged_maxpool(const float* x, int64_t x_pixels, float* y, int64_t y_pixels, const hsefr_ragged_map* d_maps, int n_items,
                         const int32_t* d_block_item, int n_blocks, int c, int k, int stride, void* stream);

/*
 * Stage 1 of every frame in one launch, one workgroup per frame: the frame's items in level order through the body of
 * hsefr_mtcnn_stage1_level (a workgroup barrier between levels), then the body of hsefr_mtcnn_stage1_finish with the frame's own
 * w, h.  found [n_frames, cap, 9], counters int32 [n_frames, 8] (zeroed by the caller), boxes [n_frames, cap, 5], tab int32
 * [n_frames, cap, 8]: per frame what the single-frame entries write.  prob [n_cells, 2], reg [n_cells, 4].  A frame without items
 * gets count 0.
 */
int hsefr_ragged_stage1(const float* prob, const float* reg, int64_t n_cells, const hsefr_ragged_frame* d_frame_tab, int n_frames,
                        const hsefr_ragged_cells* d_cells, int n_items, float thr, double* found, int32_t* counters, double* boxes,
                        int32_t* tab, void* stream);

/* hsefr_mtcnn_crops_batch with the frame's place and size from the frame table: crop k of the list [n, size, size, 3] belongs to the
 * frame b with offsets[b] <= k < offsets[b + 1] and is row k - offsets[b] of tables [n_frames, rows, 8] */
int hsefr_ragged_crops(const uint8_t* d_frames, int64_t frames_bytes, const hsefr_ragged_frame* d_frame_tab, int n_frames, const int32_t* tables,
                       const int32_t* offsets, float* dst, int rows, int n, int size, void* stream);

/* hsefr_mtcnn_stage_finish_batch (stage 2 or 3) with every frame's img_w, img_h from the frame table */
int hsefr_ragged_stage_finish(int stage, const double* boxes_in, const int32_t* offsets, int n_total, const float* prob, const float* reg,
                              const float* pts, float thr, double* boxes_out, int32_t* tab_out, float* points_out, int32_t* counters,
                              const hsefr_ragged_frame* d_frame_tab, int n_frames, void* stream);

#ifdef __cplusplus
}
#endif

#endif
