// libhsefr_album.so (include/hsefr_album.h): the faces of a pass of frames, cut and resized from the frame stack on the device.
//
// process_photos.py:38 resizes every face crop to 224 x 224 with cv2.resize; until this file the crops were cut on the host from frames
// the detector had already uploaded, grouped by crop size, and resized one size per launch (preprocess_device.preprocess_faces_cv).
// Here one launch covers every box of the pass: a workgroup computes its box's taps itself and gathers from the frame stack.
//
// The taps are computed in the kernel, not uploaded: a table would be (oh + ow) * 12 bytes per face built by a host loop per face,
// which is the loop this file removes; the arithmetic is short and exactly reproducible -- preprocess_device.cv_linear_taps is
//   pos  = (float)(((double)o + 0.5) * ((double)in / (double)out) - 0.5)      product and difference rounded separately
//   base = floor(pos); frac = pos - base, 0 at the clamped borders; w1 = rint(frac * 2048)
// IEEE double division, multiplication and subtraction and the float conversion round the same on the device as in NumPy as long as
// the compiler does not fuse the product with the subtraction: contraction is off for this file (the pragma below, and the flag
// csrc/build.sh adds for it).
//
// The tap and the blend of one output byte live in cv_linear_px.h, which mixed_frames.hip (libhsefr_mixed.so: the same crops from a packed
// buffer of frames of different sizes) compiles too.
//
// Shared with libhsefr.so: no symbol (it is linked with -fvisibility=hidden; this library has its own error string).
#include <hip/hip_runtime.h>

#include "../../include/hsefr_album.h"
#include "lib_error.h"

#pragma clang fp contract(off)

#include "cv_linear_px.h"

using namespace hsefr;      // linear_tap, linear_blend (cv_linear_px.h, shared with mixed_frames.hip); g_error, set_error (lib_error.h)

#define ALBUM_REQUIRE HSEFR_LIB_REQUIRE
#define ALBUM_HIP_CHECK(expr) HSEFR_LIB_HIP_CHECK(expr, HSEFR_ALBUM_ERR_NOMEM, HSEFR_ALBUM_ERR_HIP)

namespace {

constexpr int UNITS_PER_BLOCK = 1024;      // 16-byte pieces (or single bytes) of one face's output per workgroup: four per thread
constexpr int MAX_TAPS = 4096;             // oh + ow: the two tap tables of a workgroup, 12 bytes per entry, in LDS

// VEC: a thread writes 16 consecutive bytes of its face's [oh, ow, 3] output with one store (the face's byte count is a multiple of
// 16 and `out` is 16-byte aligned: 224 x 224 x 3 rows are 42 such stores); otherwise one byte per thread.  Every output byte is the
// two-stage fixed-point blend of four source bytes; neighbouring bytes share them, so the loads are served by the vector L1 and L2.
template <bool VEC>
__global__ __launch_bounds__(256) void face_crops_kernel(const unsigned char* __restrict__ frames, const int* __restrict__ boxes,
                                                         unsigned char* __restrict__ out, int h, int w, int oh, int ow, int units,
                                                         int blocks_per_face) {
    extern __shared__ __attribute__((aligned(16))) int taps[];
    int* xo0 = taps;                 // [ow] byte offset of the left source pixel in its row
    int* xo1 = xo0 + ow;             // [ow] ... of the right one
    int* xw1 = xo1 + ow;             // [ow] weight of the right one
    int* yr0 = xw1 + ow;             // [oh] upper source row
    int* yr1 = yr0 + oh;             // [oh] lower source row
    int* yw1 = yr1 + oh;             // [oh] weight of the lower one
    const int tid = threadIdx.x;
    const int face = blockIdx.x / blocks_per_face, part = blockIdx.x - face * blocks_per_face;
    const int* box = boxes + (long long)face * 5;
    const int f = box[0], bx = box[1], by = box[2], bw = box[3] - box[1], bh = box[4] - box[2];
    for (int i = tid; i < ow + oh; i += 256) {
        int i0, i1, w1;
        if (i < ow) {
            linear_tap(i, bw, ow, i0, i1, w1);
            xo0[i] = i0 * 3; xo1[i] = i1 * 3; xw1[i] = w1;
        } else {
            linear_tap(i - ow, bh, oh, i0, i1, w1);
            yr0[i - ow] = i0; yr1[i - ow] = i1; yw1[i - ow] = w1;
        }
    }
    __syncthreads();
    const long long wrow = (long long)w * 3;
    const int rowb = ow * 3;
    const unsigned char* src = frames + ((long long)f * h + by) * wrow + (long long)bx * 3;
    unsigned char* dst = out + (long long)face * oh * rowb;
    const int last = min((part + 1) * UNITS_PER_BLOCK, units);
    for (int u = part * UNITS_PER_BLOCK + tid; u < last; u += 256) {
        const int g = VEC ? u * 16 : u;
        int y = g / rowb;
        int b = g - y * rowb;
        int x = b / 3;
        int c = b - 3 * x;
        unsigned word[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < (VEC ? 16 : 1); ++k) {
            const unsigned v = linear_blend(src + yr0[y] * wrow + c, src + yr1[y] * wrow + c, xo0[x], xo1[x], xw1[x], yw1[y]);
            if (VEC) {
                word[k >> 2] |= v << (8 * (k & 3));
                if (++c == 3) { c = 0; ++x; }
                if (++b == rowb) { b = 0; x = 0; c = 0; ++y; }
            } else {
                dst[g] = (unsigned char)v;
            }
        }
        if (VEC) {
            *reinterpret_cast<uint4*>(dst + g) = make_uint4(word[0], word[1], word[2], word[3]);
            asm volatile("s_nop 1" ::: "memory");      // gfx950 store-data hazard: two wait states behind a 16-byte store (tools/isa_lint.py)
        }
    }
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int hsefr_album_version(void) { return HSEFR_ALBUM_VERSION; }

__attribute__((visibility("default"))) const char* hsefr_album_last_error_string(void) { return g_error; }

__attribute__((visibility("default"))) int hsefr_album_face_crops(const uint8_t* frames, int n_frames, int h, int w, const int* boxes, int m,
                                                                   uint8_t* out, int oh, int ow, void* stream) {
    ALBUM_REQUIRE(m >= 0, HSEFR_ALBUM_ERR_INVALID, "face_crops: m = %d", m);
    if (m == 0) return HSEFR_ALBUM_OK;
    ALBUM_REQUIRE(frames && boxes && out, HSEFR_ALBUM_ERR_INVALID, "face_crops: null %s pointer with m = %d",
                  !frames ? "frames" : (!boxes ? "boxes" : "out"), m);
    ALBUM_REQUIRE(n_frames > 0 && h > 0 && w > 0, HSEFR_ALBUM_ERR_INVALID, "face_crops: bad frame stack [%d, %d, %d, 3]", n_frames, h, w);
    ALBUM_REQUIRE(oh > 0 && ow > 0, HSEFR_ALBUM_ERR_INVALID, "face_crops: bad output size %d x %d", oh, ow);
    for (int i = 0; i < m; ++i) {
        const int* b = boxes + (size_t)i * 5;
        ALBUM_REQUIRE(b[0] >= 0 && b[0] < n_frames, HSEFR_ALBUM_ERR_INVALID, "face_crops: box %d names frame %d of %d", i, b[0], n_frames);
        ALBUM_REQUIRE(b[3] > b[1] && b[4] > b[2], HSEFR_ALBUM_ERR_INVALID, "face_crops: box %d is empty (x %d..%d, y %d..%d)", i, b[1], b[3],
                      b[2], b[4]);
        ALBUM_REQUIRE(b[1] >= 0 && b[2] >= 0 && b[3] <= w && b[4] <= h, HSEFR_ALBUM_ERR_INVALID,
                      "face_crops: box %d (x %d..%d, y %d..%d) is outside the %d x %d frame", i, b[1], b[3], b[2], b[4], w, h);
    }
    ALBUM_REQUIRE(oh + ow <= MAX_TAPS, HSEFR_ALBUM_ERR_UNSUPPORTED, "face_crops: output %d x %d (the tap tables hold %d entries)", oh, ow,
                  MAX_TAPS);
    const long long face_bytes = (long long)oh * ow * 3;
    ALBUM_REQUIRE(face_bytes < (1ll << 31), HSEFR_ALBUM_ERR_UNSUPPORTED, "face_crops: output %d x %d too large", oh, ow);
    const bool vec = face_bytes % 16 == 0 && ((uintptr_t)out & 15) == 0;
    const int units = (int)(vec ? face_bytes / 16 : face_bytes);
    const int blocks_per_face = (units + UNITS_PER_BLOCK - 1) / UNITS_PER_BLOCK;
    ALBUM_REQUIRE((long long)m * blocks_per_face < (1ll << 31), HSEFR_ALBUM_ERR_UNSUPPORTED, "face_crops: %d faces of %d x %d: too many", m, oh, ow);
    // the table's device copy lives from here to the end of the launch, both in stream order: no allocation outlives the call and the
    // device is not synchronised
    hipStream_t s = (hipStream_t)stream;
    const size_t table_bytes = (size_t)m * 5 * sizeof(int);
    int* d_boxes = nullptr;
    ALBUM_HIP_CHECK(hipMallocAsync((void**)&d_boxes, table_bytes, s));
    hipError_t e = hipMemcpyAsync(d_boxes, boxes, table_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        const dim3 grid((unsigned)((long long)m * blocks_per_face)), block(256);
        const size_t lds = (size_t)(oh + ow) * 3 * sizeof(int);
        if (vec)
            hipLaunchKernelGGL(face_crops_kernel<true>, grid, block, lds, s, frames, d_boxes, out, h, w, oh, ow, units, blocks_per_face);
        else
            hipLaunchKernelGGL(face_crops_kernel<false>, grid, block, lds, s, frames, d_boxes, out, h, w, oh, ow, units, blocks_per_face);
        e = hipGetLastError();
    }
    const hipError_t e_free = hipFreeAsync(d_boxes, s);
    if (e == hipSuccess) e = e_free;
    if (e != hipSuccess) {
        set_error("face_crops: %s", hipGetErrorString(e));
        return HSEFR_ALBUM_ERR_HIP;
    }
    return HSEFR_ALBUM_OK;
}

}  // extern "C"
