/*
 * hsefr_frames.h -- C ABI of libhsefr_frames.so, the front end of the album organiser's device path
 * (hse_facerec_tf_amd/album.py, FacialImageProcessing.process_images; the reference's age_gender_identity/process_photos.py).
 *
 * What it replaces in the reference:
 *   - cv2.cvtColor(draw, cv2.COLOR_BGR2RGB) per frame                      facial_analysis.py:226
 *   - cv2.flip(cv2.transpose(frame), 1 or 0) per turned frame              process_photos.py:102-107, :242-247
 *       -> hsefr_frames_prepare(): a pass's frames, uploaded as decoded (BGR, unrotated), written as the RGB stack turned upright
 *          in one launch; the detector and the crop kernel read that stack
 *
 * A library of its own, as libhsefr_album.so is: libhsefr.so stays as it is (its size is bounded by its tests) and the three share
 * no symbol -- this one has its own version number and its own per-thread error string.
 *
 * Conventions: those of hsefr.h -- extern "C", plain C types, 0 on success or a negative status (the values of hsefr_status), never
 * throws, data pointers are DEVICE pointers owned by the caller, launches are asynchronous on `stream` (a hipStream_t passed as
 * void*; NULL = the default stream).  Built for gfx950 only.
 */
#ifndef HSEFR_FRAMES_H
#define HSEFR_FRAMES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSEFR_FRAMES_VERSION 100

#define HSEFR_FRAMES_OK 0
#define HSEFR_FRAMES_ERR_INVALID (-1)     /* bad argument                              */
#define HSEFR_FRAMES_ERR_UNSUPPORTED (-2) /* a size the kernel does not cover          */
#define HSEFR_FRAMES_ERR_HIP (-3)         /* a HIP runtime call failed                 */

int hsefr_frames_version(void);

/* the last failure on the calling thread ("" before the first) */
const char* hsefr_frames_last_error_string(void);

/*
 * d_dst[i] = d_src[i] turned by `rotation` degrees clockwise, with channels 0 and 2 exchanged when swap_rb != 0 -- pure data movement,
 * byte for byte NumPy's
 *   rotation   0 : x                     d_dst uint8 [n, h, w, 3]
 *   rotation  90 : np.rot90(x, -1)       d_dst uint8 [n, w, h, 3]     (cv2.flip(cv2.transpose(x), 1): a quarter turn clockwise)
 *   rotation 270 : np.rot90(x, 1)        d_dst uint8 [n, w, h, 3]     (cv2.flip(cv2.transpose(x), 0): a quarter turn counter-clockwise)
 * followed by [..., ::-1] for swap_rb.
 *   d_src   DEVICE uint8 [n, h, w, 3]
 * Every argument is checked before any device work; HSEFR_FRAMES_ERR_INVALID for a rotation outside {0, 90, 270}, n < 0, h or w
 * below 1, a null pointer with n > 0 and d_dst == d_src with a quarter turn; HSEFR_FRAMES_ERR_UNSUPPORTED for a frame of 2^31
 * bytes or more.  d_dst == d_src with rotation 0 is allowed: the exchange then runs in place (every thread writes the bytes it
 * read).  Two stacks that overlap in any other way are not supported and not detected.  With n == 0 the rotation and the frame size
 * are still checked; then the call returns 0 and does nothing, whatever the pointers.  One launch for any n.  No alignment is asked
 * of either pointer or of the sizes: rows and frames that do not start on a 4-byte boundary take a byte path, which writes exactly
 * the bytes of d_dst and no other.
 */
int hsefr_frames_prepare(const uint8_t* d_src, uint8_t* d_dst, int n, int h, int w, int rotation, int swap_rb, void* stream);

#ifdef __cplusplus
}
#endif

#endif
