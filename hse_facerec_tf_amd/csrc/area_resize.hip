// cv2.resize(..., interpolation=cv2.INTER_AREA) on the device, for the two places the MTCNN cascade of the reference uses
// it (facial_analysis.py:507 -- the image pyramid --, :546 and :575 -- the 24x24 / 48x48 crops fed to R-Net / O-Net), with
// the normalisation (v - 127.5) * 0.0078125 and the (W, H) transposition the nets are fed with fused in.
//
// Host restatement: hse_facerec_tf_amd/preprocess.py resize_area (tables of _area_weights / _area_linear_taps); the
// same coverage weights are derived here per output coordinate instead of being tabulated.
//   pyramid level : uint8 frame -> uint8-rounded level (OpenCV's 8-bit path: float32 accumulation, horizontal taps first,
//                   then vertical, first tap assigns; 2x2 and integer-factor box special cases; bilinear fixed point
//                   when enlarging) -> normalised float32, written transposed [W', H', 3];
//   crops         : per box, the box-sized tile of the frame (zero outside the frame) resized to S x S in float64 (the
//                   reference resizes a float64 tile), normalised, written transposed [n, S, S, 3].
// Arithmetic is kept un-contracted (explicit mul / add) so that the order of roundings is the restatement's.
#include <cmath>

#include "common.h"
#include "area_resize_px.h"      // the one-frame bodies (shared with mtcnn_ragged.hip): area_level_pixel, area_level_row, area_crop_pixel

namespace hsefr {

namespace {

// ---- pyramid level: uint8 [H,W,3] -> float32 [dw,dh,3] (transposed), value = (u8(resized) - 127.5) * 0.0078125 ---------------
// blockIdx.y is the frame of a stack of same-size frames [B,H,W,3] -> [B,dw,dh,3] (one frame: a grid of height 1): a frame's pixels
// come from that frame alone, by the operations below in their order, whatever stands next to it.
__global__ __launch_bounds__(256) void area_level_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, int sh, int sw, int dh,
                                                         int dw) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= dh * dw) return;
    src += (size_t)blockIdx.y * sh * sw * 3;
    dst += (size_t)blockIdx.y * dh * dw * 3;
    area_level_pixel(src, dst, sh, sw, dh, dw, i);
}

// The general decimation case row by row (area_level_row, area_resize_px.h): blockIdx.x is the destination row
__global__ __launch_bounds__(256) void area_level_rows_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, int sh, int sw,
                                                              int dh, int dw, int hoff) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    src += (size_t)blockIdx.y * sh * sw * 3;                                   // the frame of a stack, as in area_level_kernel
    dst += (size_t)blockIdx.y * dh * dw * 3;
    area_level_row(src, dst, sh, sw, dh, dw, hoff, blockIdx.x, lds);
}

// One frame (offsets == nullptr): crop k is row k of the table `boxes` [n, 8].  A stack of B same-size frames with the crops of all
// frames as ONE list [n, S, S, 3]: crop k belongs to the frame b with offsets[b] <= k < offsets[b + 1] and is row k - offsets[b] of that
// frame's table (tables [B, rows, 8]); offsets [B + 1] ascending from 0 to n, and a crop whose frame or row cannot be found there (a
// malformed list) is left unwritten.  (One kernel for both: the product library has no room for the body twice, tests/test_abi_cpu.py.)
__global__ __launch_bounds__(256) void area_crops_kernel(const unsigned char* __restrict__ src, const int* __restrict__ boxes,
                                                         const int* __restrict__ offsets, float* __restrict__ dst, int B, int rows, int sh,
                                                         int sw, int n, int S) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n * S * S) return;
    const int k = (int)(i / (S * S)), rem = (int)(i - (long long)k * S * S), dy = rem / S, dx = rem - dy * S;
    const int* bx = boxes + k * 8;
    if (offsets) {
        int lo = 0, hi = B;                                                   // the last b with offsets[b] <= k
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (offsets[mid] <= k) lo = mid; else hi = mid;
        }
        const int row = k - offsets[lo];
        if (row < 0 || row >= rows || k >= offsets[lo + 1]) return;
        src += (size_t)lo * sh * sw * 3;
        bx = boxes + ((size_t)lo * rows + row) * 8;
    }
    area_crop_pixel(src, bx, dst + (((long long)k * S + dx) * S + dy) * 3, sw, S, dy, dx);   // transposed: the nets see (W, H)
}

}  // namespace

int launch_area_level(const unsigned char* src, float* dst, int sh, int sw, int dh, int dw, hipStream_t s) {
    return launch_area_level_batch(src, dst, 1, sh, sw, dh, dw, s);
}

int launch_area_level_batch(const unsigned char* src, float* dst, int frames, int sh, int sw, int dh, int dw, hipStream_t s) {
    HSEFR_REQUIRE(sh > 0 && sw > 0 && dh > 0 && dw > 0, HSEFR_ERR_INVALID, "area_level: bad shape");
    HSEFR_REQUIRE(frames >= 1 && frames <= 65535, HSEFR_ERR_INVALID, "area_level: %d frames (1 .. 65535)", frames);
    // the general decimation case (both factors >= 1, not both integers: every level of MTCNN's 0.709 pyramid) row by row
    const double fx = (double)sw / dw, fy = (double)sh / dh;
    if (fx >= 1.0 && fy >= 1.0 && !(sh == dh && sw == dw)) {
        const double eps = 2.220446049250313e-16;
        const bool integer = std::fabs(fx - std::rint(fx)) < eps && std::fabs(fy - std::rint(fy)) < eps;
        const size_t hoff = area_rows_hoff(dw), lds = area_rows_lds(dw, fy);
        if (!integer && lds <= 64 * 1024) {
            HSEFR_LAUNCH(area_level_rows_kernel, dim3(dh, frames), dim3(256), lds, s, src, dst, sh, sw, dh, dw, (int)hoff);
            return launch_status("area_level_rows");
        }
    }
    HSEFR_LAUNCH(area_level_kernel, dim3((dh * dw + 255) / 256, frames), dim3(256), 0, s, src, dst, sh, sw, dh, dw);
    return launch_status("area_level");
}

int launch_area_crops(const unsigned char* src, const int* boxes, float* dst, int sh, int sw, int n, int size, hipStream_t s) {
    HSEFR_REQUIRE(sh > 0 && sw > 0 && n >= 0 && size > 0, HSEFR_ERR_INVALID, "area_crops: bad shape");
    if (n == 0) return HSEFR_OK;
    const long long total = (long long)n * size * size;
    HSEFR_LAUNCH(area_crops_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, boxes, (const int*)nullptr, dst, 1, n, sh, sw, n,
                 size);
    return launch_status("area_crops");
}

int launch_area_crops_batch(const unsigned char* frames, const int* tables, const int* offsets, float* dst, int n_frames, int rows, int sh, int sw,
                            int n, int size, hipStream_t s) {
    HSEFR_REQUIRE(n_frames >= 1 && rows > 0 && sh > 0 && sw > 0 && n >= 0 && size > 0, HSEFR_ERR_INVALID, "area_crops_batch: bad shape");
    // the kernel indexes a frame's bytes, the tables' rows and a crop's position in the list with int
    HSEFR_REQUIRE((long long)sh * sw * 3 < (1ll << 31) && (long long)n_frames * rows < (1ll << 31) && (long long)size * size < (1ll << 31),
                  HSEFR_ERR_UNSUPPORTED, "area_crops_batch: %d frames of %dx%d with %d table rows, size %d: an index leaves 31 bits", n_frames, sh, sw,
                  rows, size);
    if (n == 0) return HSEFR_OK;
    const long long total = (long long)n * size * size;
    HSEFR_REQUIRE((total + 255) / 256 < (1ll << 31), HSEFR_ERR_UNSUPPORTED, "area_crops_batch: %d crops of size %d", n, size);
    HSEFR_LAUNCH(area_crops_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, frames, tables, offsets, dst, n_frames, rows, sh, sw, n,
                 size);
    return launch_status("area_crops_batch");
}

}  // namespace hsefr
