// The per-pixel device bodies of cv2.resize(..., INTER_LINEAR) on 8-bit images: one output coordinate's taps and one output byte's
// two-stage fixed-point blend.  album.hip (libhsefr_album.so: crops from a same-size stack) and mixed_frames.hip (libhsefr_mixed.so:
// crops from a packed buffer of frames of different sizes) compile this same code, so a crop's bytes are the same whichever entry cut it.
//
// preprocess_device.cv_linear_taps is
//   pos  = (float)(((double)o + 0.5) * ((double)in / (double)out) - 0.5)      product and difference rounded separately
//   base = floor(pos); frac = pos - base, 0 at the clamped borders; w1 = rint(frac * 2048)
// IEEE double division, multiplication and subtraction and the float conversion round the same on the device as in NumPy as long as
// the compiler does not fuse the product with the subtraction: contraction is off from here on (the pragma below, and the flag
// csrc/build.sh adds for every source that includes this file).
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace hsefr {

namespace {

// one output coordinate: the two source indices and the 11-bit weight of the second
__device__ __forceinline__ void linear_tap(int o, int n_in, int n_out, int& i0, int& i1, int& w1) {
    const double scale = (double)n_in / (double)n_out;
    const double prod = ((double)o + 0.5) * scale;
    const float pos = (float)(prod - 0.5);
    const float fl = floorf(pos);
    int base = (int)fl;
    float frac = pos - fl;
    if (base < 0 || base >= n_in - 1) frac = 0.f;
    base = min(max(base, 0), n_in - 1);
    i0 = base;
    i1 = min(base + 1, n_in - 1);
    w1 = (int)rintf(frac * 2048.f);
}

// one output byte: r0 / r1 point at the channel's byte in the first pixel of the upper / lower source row, x0 / x1 are the byte offsets
// of the left / right source pixel in a row, a1 / b1 the weights of the right pixel / the lower row.  At most 255: the weights of a pair
// sum to 2048
__device__ __forceinline__ unsigned linear_blend(const unsigned char* r0, const unsigned char* r1, int x0, int x1, int a1, int b1) {
    const int a0 = 2048 - a1, b0 = 2048 - b1;
    const int s0 = r0[x0] * a0 + r0[x1] * a1;
    const int s1 = r1[x0] * a0 + r1[x1] * a1;
    return (unsigned)((((b0 * (s0 >> 4)) >> 16) + ((b1 * (s1 >> 4)) >> 16) + 2) >> 2) & 255u;
}

}  // namespace

}  // namespace hsefr
