/*
 * hsefr_album.h -- C ABI of libhsefr_album.so, the device half of the album organiser
 * (hse_facerec_tf_amd/album.py; the reference's age_gender_identity/process_photos.py).
 *
 * What it replaces in the reference:
 *   - cv2.resize(img[y1:y2, x1:x2, :], (224, 224)) per face      process_photos.py:38 ; facial_analysis.py:95
 *       -> hsefr_album_face_crops(): every face of a pass of frames, cut and resized from the frame stack the detector left on
 *          the device, in one launch
 *
 * A library of its own: libhsefr.so stays as it is (its size is bounded by its tests), and the two share no symbol -- this one has
 * its own version number and its own per-thread error string.
 *
 * Conventions: those of hsefr.h -- extern "C", plain C types, 0 on success or a negative status (the values of hsefr_status), never
 * throws, data pointers are DEVICE pointers owned by the caller, launches are asynchronous on `stream` (a hipStream_t passed as
 * void*; NULL = the default stream).  The one exception is named at its argument: the box table of hsefr_album_face_crops is a HOST
 * pointer, because the function checks every box before any device work.  Built for gfx950 only.
 */
#ifndef HSEFR_ALBUM_H
#define HSEFR_ALBUM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSEFR_ALBUM_VERSION 100

#define HSEFR_ALBUM_OK 0
#define HSEFR_ALBUM_ERR_INVALID (-1)     /* bad argument                              */
#define HSEFR_ALBUM_ERR_UNSUPPORTED (-2) /* a size the kernel does not cover          */
#define HSEFR_ALBUM_ERR_HIP (-3)         /* a HIP runtime call failed                 */
#define HSEFR_ALBUM_ERR_NOMEM (-4)       /* the device copy of the box table          */

int hsefr_album_version(void);

/* the last failure on the calling thread ("" before the first) */
const char* hsefr_album_last_error_string(void);

/*
 * out[i] = cv2.resize(frames[f][y1:y2, x1:x2, :], (ow, oh)) with the default INTER_LINEAR, byte for byte (OpenCV's 8-bit path: 11-bit
 * tap weights, two-stage rounding; preprocess.resize_linear_u8 is the package's restatement), for box i = (f, x1, y1, x2, y2) with
 * x2, y2 exclusive.  Channel order is kept.
 *   frames  DEVICE uint8 [n_frames, h, w, 3]
 *   boxes   HOST   int32 [m, 5]; read and checked here, then copied to the device on `stream` (one copy; the caller's table may be
 *           freed or changed as soon as the call returns)
 *   out     DEVICE uint8 [m, oh, ow, 3]
 * Every argument is checked before any device work; HSEFR_ALBUM_ERR_INVALID for a null pointer with m > 0, a non-positive size,
 * a frame index outside [0, n_frames), an empty box (x2 <= x1 or y2 <= y1) and a box that leaves its frame.  m == 0 returns 0 and
 * does nothing.  One launch for any m; the taps of a box are computed in the kernel.
 */
int hsefr_album_face_crops(const uint8_t* frames, int n_frames, int h, int w, const int* boxes, int m, uint8_t* out, int oh, int ow,
                           void* stream);

#ifdef __cplusplus
}
#endif

#endif
