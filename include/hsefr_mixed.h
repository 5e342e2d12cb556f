/*
 * hsefr_mixed.h -- C ABI of libhsefr_mixed.so: the two device stages of a mixed-size detector pass
 * (hse_facerec_tf_amd/album.py, FacialImageProcessing.process_images(mixed_device=True); the reference's
 * age_gender_identity/process_photos.py).
 *
 * What it replaces in the reference, for frames of DIFFERENT sizes that share one pass (hsefr_ragged.h):
 *   - cv2.cvtColor(draw, cv2.COLOR_BGR2RGB) per frame                      facial_analysis.py:226
 *   - cv2.flip(cv2.transpose(frame), 1 or 0) per turned frame              process_photos.py:102-107, :242-247
 *       -> hsefr_mixed_frames_prepare(): what hsefr_frames_prepare (hsefr_frames.h) does for a same-size stack, for every frame of a
 *          packed buffer in one launch
 *   - cv2.resize(frame[y1:y2, x1:x2], (224, 224)) per face                 process_photos.py:38
 *       -> hsefr_mixed_face_crops(): what hsefr_album_face_crops (hsefr_album.h) does for a same-size stack, with a place and a
 *          size per frame
 *
 * A library of its own, as the four before it: libhsefr.so stays as it is (its size is bounded by its tests) and the six share no
 * symbol -- this one has its own version number and its own per-thread error string.  Its per-pixel device code is the code of
 * libhsefr_frames.so and libhsefr_album.so (csrc/frames_px.h, csrc/cv_linear_px.h), compiled twice.
 *
 * Conventions: those of hsefr.h -- extern "C", plain C types, 0 on success or a negative status (the values of hsefr_status), never
 * throws, data pointers are DEVICE pointers owned by the caller, launches are asynchronous on `stream` (a hipStream_t passed as
 * void*; NULL = the default stream).  The frame table and the box table are HOST pointers: the library checks every row before any
 * device work and uploads what its kernels need itself, in stream order (hipMallocAsync / hipMemcpyAsync / hipFreeAsync): the
 * device is not synchronised and no allocation outlives the call.  Built for gfx950 only.
 */
#ifndef HSEFR_MIXED_H
#define HSEFR_MIXED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSEFR_MIXED_VERSION 100

#define HSEFR_MIXED_OK 0
#define HSEFR_MIXED_ERR_INVALID (-1)     /* bad argument                              */
#define HSEFR_MIXED_ERR_UNSUPPORTED (-2) /* a size the kernels do not cover           */
#define HSEFR_MIXED_ERR_HIP (-3)         /* a HIP runtime call failed                 */
#define HSEFR_MIXED_ERR_NOMEM (-4)       /* the tables' device copy did not fit       */

/* A frame of a packed buffer: uint8 [h, w, 3] at byte `offset`.  Any offset will do (mtcnn.ragged_plan puts frames back to back, so
 * odd ones are usual).  A table is valid for a buffer of buffer_bytes if every row has offset >= 0, h and w >= 1, h * w * 3 < 2^31
 * and offset + h * w * 3 <= buffer_bytes, and no two frames overlap; rows may stand in any order, with gaps between frames. */
typedef struct { int64_t offset; int32_t h, w; } hsefr_mixed_frame;   /* 16 bytes */

int hsefr_mixed_version(void);

/* the last failure on the calling thread ("" before the first) */
const char* hsefr_mixed_last_error_string(void);

/*
 * hsefr_frames_prepare for every frame of a packed buffer, in ONE launch: frame i, read from d_src + frames[i].offset as
 * uint8 [h, w, 3], is written at the SAME offset of d_dst, turned by `rotation` degrees clockwise, with channels 0 and 2 exchanged
 * when swap_rb != 0 -- pure data movement, byte for byte NumPy's
 *   rotation   0 : x                     written as [h, w, 3]
 *   rotation  90 : np.rot90(x, -1)       written as [w, h, 3]
 *   rotation 270 : np.rot90(x, 1)        written as [w, h, 3]
 * followed by [..., ::-1] for swap_rb.  The table gives the SOURCE sizes.
 *   d_src, d_dst   DEVICE uint8 [buffer_bytes]
 *   frames         HOST [n_frames]
 * No byte of d_dst outside the frames' own ranges is written: not between frames, not before the first, not after the last.
 * d_dst == d_src with rotation 0 is allowed (every thread writes the bytes it read); buffers that overlap in any other way are not
 * supported and not detected.  HSEFR_MIXED_ERR_INVALID for a rotation outside {0, 90, 270}, n_frames or buffer_bytes below 0, a null
 * pointer with n_frames > 0, d_dst == d_src with a quarter turn, and a table that is not valid (above) except for a frame of 2^31
 * bytes or more, which is HSEFR_MIXED_ERR_UNSUPPORTED.  With n_frames == 0 the scalars are still checked; then the call returns 0
 * and does nothing, whatever the pointers.  No alignment is asked of the pointers, the offsets or the sizes: whether a frame's rows
 * are read, and its turned rows written, as 12-byte units or byte by byte is decided per frame and per side from its address
 * (pointer + offset) and its size.
 */
int hsefr_mixed_frames_prepare(const uint8_t* d_src, uint8_t* d_dst, int64_t buffer_bytes, const hsefr_mixed_frame* frames, int n_frames,
                               int rotation, int swap_rb, void* stream);

/*
 * hsefr_album_face_crops with a place and a size per frame: d_out[i] = cv2.resize(frame[y1:y2, x1:x2], (ow, oh)) (INTER_LINEAR, the
 * 8-bit path: the same taps and the same two-stage fixed-point blend), byte for byte, channel order kept, for every row
 * i = (frame, x1, y1, x2, y2) of `boxes` (x2, y2 exclusive), in ONE launch.
 *   d_frames   DEVICE uint8 [buffer_bytes]: the packed frames (what hsefr_mixed_frames_prepare wrote, or an upload)
 *   frames     HOST [n_frames]: the frames AS THEY STAND in d_frames (after a quarter turn: h and w exchanged)
 *   boxes      HOST int32 [m, 5]; rows in any order, any number per frame
 *   d_out      DEVICE uint8 [m, oh, ow, 3]
 * HSEFR_MIXED_ERR_INVALID for m, n_frames or buffer_bytes below 0, a null pointer with m > 0, oh or ow below 1, a table that is not
 * valid, a box that names a frame outside 0 .. n_frames - 1, is empty, or does not lie inside ITS frame's h and w;
 * HSEFR_MIXED_ERR_UNSUPPORTED for oh + ow above 4096 (the tap tables of a workgroup) and counts that pass 31 bits.  With m == 0 the
 * call returns 0 and does nothing, whatever else it was given.  Where oh * ow * 3 is a multiple of 16 and d_out is 16-byte aligned
 * a thread stores 16 bytes at a time; otherwise byte by byte.
 */
int hsefr_mixed_face_crops(const uint8_t* d_frames, int64_t buffer_bytes, const hsefr_mixed_frame* frames, int n_frames, const int32_t* boxes,
                           int m, uint8_t* d_out, int oh, int ow, void* stream);

#ifdef __cplusplus
}
#endif

#endif
