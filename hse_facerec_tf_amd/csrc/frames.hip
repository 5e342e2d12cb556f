// libhsefr_frames.so (include/hsefr_frames.h): a pass's frames as decoded -- BGR, unrotated -- written as the RGB stack, turned upright.
//
// process_photos.py turns a photo with cv2.flip(cv2.transpose(x), .) (:102-107, :242-247) and facial_analysis.py:226 converts every
// frame with cv2.cvtColor; until this file both were host copies of every pixel (album._rotate, FacialImageProcessing._bgr_to_rgb) of
// frames that were uploaded right after.  Both only permute bytes, so here they are one launch over the uploaded stack.
//
// Two kernels, both pure data movement:
//   swap_kernel   rotation 0.  A lane takes 4 pixels = 12 bytes: one 12-byte load, the bytes permuted in registers, one 12-byte store.
//                 A lane writes exactly the bytes it read, so the stack may be its own destination.
//   turn_kernel   rotations 90 and 270.  A 64 x 64 pixel tile goes through LDS, one dword per pixel, stored TRANSPOSED
//                 (tile[column][row]): global reads run along source rows (a lane loads 12 bytes, 16 lanes cover a tile row), global
//                 writes along destination rows (a lane reads its 4 pixels as one ds_read_b128 and stores 12 bytes).  An LDS row is
//                 64 + 4 dwords: 16-byte aligned for the wide read, and with the load phase's lane mapping (16 rows x 2 chunks per
//                 half wave) the 32 transposed dword writes of a half wave fall on 32 different banks: (4j + k) * 68 + r = 16 j + r
//                 + const (mod 32).
// Each has a byte path per side (template flags): rows or frames that do not start on a 4-byte boundary (w or h not a multiple of 4, an
// odd pointer) are read and written byte by byte, one pixel per lane, and edge tiles are cut by predicates: no byte outside the
// destination stack is written.
//
// The per-pixel bodies (a pixel as a dword, the 12-byte unit and its guarded store, the byte forms) live in frames_px.h, which
// mixed_frames.hip (libhsefr_mixed.so: the same work over a packed buffer of frames of different sizes) compiles too.
//
// Shared with libhsefr.so and libhsefr_album.so: no symbol (linked with -fvisibility=hidden; this library has its own error string).
#include <hip/hip_runtime.h>

#include "../../include/hsefr_frames.h"
#include "frames_px.h"
#include "lib_error.h"

// Px4, unpack4, pack4, store_px4, load_pixel, store_pixel, swap_02 (frames_px.h, shared with mixed_frames.hip); g_error, set_error (lib_error.h)
using namespace hsefr;

#define FRAMES_REQUIRE HSEFR_LIB_REQUIRE

namespace {

constexpr int TILE = 64;                   // pixels per tile side
constexpr int TILE_STRIDE = TILE + 4;      // dwords per LDS row (see the head of the file)
constexpr int THREADS = 256;
constexpr int MAX_GRID_Y = 65535;
constexpr int SWAP_BLOCKS = 4096;          // rotation 0: about this many workgroups over all frames, each lane striding through its frame

// rotation 0.  VEC: both stacks 4-byte aligned and h * w a multiple of 4, so every frame is a whole number of 12-byte units that start
// on dword boundaries; otherwise one pixel per lane, byte by byte.  src and dst may be the same stack (no __restrict__): a lane reads
// its unit before it writes it and no other lane touches it.  `units`: per frame, 12-byte units or pixels.
template <bool VEC>
__global__ __launch_bounds__(THREADS) void swap_kernel(const unsigned char* src, unsigned char* dst, int n, long long frame_bytes, int units,
                                                       int swap) {
    for (int frame = blockIdx.y; frame < n; frame += gridDim.y) {
        const unsigned char* s = src + (long long)frame * frame_bytes;
        unsigned char* d = dst + (long long)frame * frame_bytes;
        for (int u = blockIdx.x * THREADS + threadIdx.x; u < units; u += gridDim.x * THREADS) {
            if (VEC) {
                const int at = u * 12;                                   // < frame_bytes < 2^31
                unsigned p[4];
                unpack4(*reinterpret_cast<const Px4*>(s + at), swap != 0, p);
                store_px4(d + at, pack4(p[0], p[1], p[2], p[3]));
            } else {
                const int at = u * 3;
                store_pixel(d + at, load_pixel(s + at, swap != 0));
            }
        }
    }
}

// rotations 90 (ccw == 0: dst[x][h - 1 - y] = src[y][x]) and 270 (ccw != 0: dst[w - 1 - x][y] = src[y][x]); dst is [n, w, h, 3].
// LOADV: src 4-byte aligned and w a multiple of 4 (every source row starts on a dword, a tile's width is a multiple of 4 pixels);
// STOREV: dst 4-byte aligned and h a multiple of 4 (the same for destination rows, whose length is h).
template <bool LOADV, bool STOREV>
__global__ __launch_bounds__(THREADS) void turn_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int n, int h,
                                                       int w, int ccw, int swap, int tiles_x) {
    __shared__ __attribute__((aligned(16))) unsigned tile[TILE * TILE_STRIDE];      // tile[source column][source row]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * TILE, y0 = ty * TILE;
    const int tw = min(TILE, w - x0), th = min(TILE, h - y0);                        // the tile's extent in the source: columns, rows
    const long long frame_bytes = (long long)h * w * 3;
    for (int frame = blockIdx.y; frame < n; frame += gridDim.y) {
        const unsigned char* s = src + (long long)frame * frame_bytes;
        unsigned char* d = dst + (long long)frame * frame_bytes;
        if (LOADV) {
            // a wave takes 16 source rows; per step, 4 chunks of 4 pixels of each: lanes 0..15 the rows of chunk j, 16..31 of j + 1, ...
            const int r = wave * 16 + (lane & 15);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = (i * 4 + (lane >> 4)) * 4;
                if (r < th && c < tw) {
                    unsigned p[4];
                    unpack4(*reinterpret_cast<const Px4*>(s + ((y0 + r) * w + x0 + c) * 3), swap != 0, p);
#pragma unroll
                    for (int k = 0; k < 4; ++k) tile[(c + k) * TILE_STRIDE + r] = p[k];
                }
            }
        } else {
            for (int i = tid; i < TILE * TILE; i += THREADS) {
                const int c = i & (TILE - 1), r = i / TILE;
                if (r < th && c < tw) tile[c * TILE_STRIDE + r] = load_pixel(s + ((y0 + r) * w + x0 + c) * 3, swap != 0);
            }
        }
        __syncthreads();
        if (STOREV) {
            // 16 lanes cover a destination row's 64 pixels of this tile, 4 pixels each; a wave takes 4 rows per step
            const int q = (lane & 15) * 4;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = i * 16 + wave * 4 + (lane >> 4);
                if (c < tw && q < th) {
                    const uint4 v = *reinterpret_cast<const uint4*>(&tile[c * TILE_STRIDE + q]);      // source rows y0 + q .. y0 + q + 3
                    if (ccw)
                        store_px4(d + ((w - 1 - x0 - c) * h + y0 + q) * 3, pack4(v.x, v.y, v.z, v.w));
                    else
                        store_px4(d + ((x0 + c) * h + (h - 4 - y0 - q)) * 3, pack4(v.w, v.z, v.y, v.x));
                }
            }
        } else {
            for (int i = tid; i < TILE * TILE; i += THREADS) {
                const int r = i & (TILE - 1), c = i / TILE;
                if (c < tw && r < th) {
                    const int row = ccw ? w - 1 - x0 - c : x0 + c, col = ccw ? y0 + r : h - 1 - y0 - r;
                    store_pixel(d + (row * h + col) * 3, tile[c * TILE_STRIDE + r]);
                }
            }
        }
        __syncthreads();                       // the next frame of this workgroup overwrites the tile
    }
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int hsefr_frames_version(void) { return HSEFR_FRAMES_VERSION; }

__attribute__((visibility("default"))) const char* hsefr_frames_last_error_string(void) { return g_error; }

__attribute__((visibility("default"))) int hsefr_frames_prepare(const uint8_t* d_src, uint8_t* d_dst, int n, int h, int w, int rotation,
                                                                 int swap_rb, void* stream) {
    FRAMES_REQUIRE(rotation == 0 || rotation == 90 || rotation == 270, HSEFR_FRAMES_ERR_INVALID, "prepare: rotation %d (0, 90 or 270)", rotation);
    FRAMES_REQUIRE(n >= 0, HSEFR_FRAMES_ERR_INVALID, "prepare: n = %d", n);
    FRAMES_REQUIRE(h >= 1 && w >= 1, HSEFR_FRAMES_ERR_INVALID, "prepare: bad frame size %d x %d", h, w);
    const long long frame_bytes = (long long)h * w * 3;
    FRAMES_REQUIRE(frame_bytes < (1ll << 31), HSEFR_FRAMES_ERR_UNSUPPORTED, "prepare: a %d x %d frame is too large (2^31 bytes or more)", h, w);
    if (n == 0) return HSEFR_FRAMES_OK;
    FRAMES_REQUIRE(d_src && d_dst, HSEFR_FRAMES_ERR_INVALID, "prepare: null %s pointer with n = %d", !d_src ? "source" : "destination", n);
    FRAMES_REQUIRE(rotation == 0 || d_dst != d_src, HSEFR_FRAMES_ERR_INVALID, "prepare: a quarter turn cannot run in place (rotation %d)",
                   rotation);
    hipStream_t s = (hipStream_t)stream;
    const bool src4 = ((uintptr_t)d_src & 3) == 0, dst4 = ((uintptr_t)d_dst & 3) == 0;
    const unsigned grid_y = (unsigned)(n < MAX_GRID_Y ? n : MAX_GRID_Y);
    if (rotation == 0) {
        const long long pixels = (long long)h * w;
        const bool vec = src4 && dst4 && pixels % 4 == 0;
        const int units = (int)(vec ? pixels / 4 : pixels);
        const int want = (units + THREADS - 1) / THREADS, cap = (SWAP_BLOCKS + (int)grid_y - 1) / (int)grid_y;
        const dim3 grid((unsigned)(want < cap ? want : cap), grid_y), block(THREADS);
        if (vec)
            hipLaunchKernelGGL(swap_kernel<true>, grid, block, 0, s, d_src, d_dst, n, frame_bytes, units, swap_rb);
        else
            hipLaunchKernelGGL(swap_kernel<false>, grid, block, 0, s, d_src, d_dst, n, frame_bytes, units, swap_rb);
    } else {
        const int tiles_x = (w + TILE - 1) / TILE, tiles_y = (h + TILE - 1) / TILE;      // at most 2^31 / 3 / 4096 tiles
        const bool loadv = src4 && w % 4 == 0, storev = dst4 && h % 4 == 0;
        const int ccw = rotation == 270;
        const dim3 grid((unsigned)(tiles_x * tiles_y), grid_y), block(THREADS);
        if (loadv && storev)
            hipLaunchKernelGGL((turn_kernel<true, true>), grid, block, 0, s, d_src, d_dst, n, h, w, ccw, swap_rb, tiles_x);
        else if (loadv)
            hipLaunchKernelGGL((turn_kernel<true, false>), grid, block, 0, s, d_src, d_dst, n, h, w, ccw, swap_rb, tiles_x);
        else if (storev)
            hipLaunchKernelGGL((turn_kernel<false, true>), grid, block, 0, s, d_src, d_dst, n, h, w, ccw, swap_rb, tiles_x);
        else
            hipLaunchKernelGGL((turn_kernel<false, false>), grid, block, 0, s, d_src, d_dst, n, h, w, ccw, swap_rb, tiles_x);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("prepare: %s", hipGetErrorString(e));
        return HSEFR_FRAMES_ERR_HIP;
    }
    return HSEFR_FRAMES_OK;
}

}  // extern "C"
