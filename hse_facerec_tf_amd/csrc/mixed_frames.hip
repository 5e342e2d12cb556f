// libhsefr_mixed.so (include/hsefr_mixed.h): the frames of a mixed-size detector pass -- different sizes, packed back to back in one
// buffer (mtcnn_ragged.ragged_plan) -- turned upright and converted to RGB, and their faces cut and resized, on the device.
//
// frames.hip and album.hip do both for a same-size stack, where a frame is a grid index; here a frame's place and size come from a
// table, as in mtcnn_ragged.hip.  The per-pixel code is theirs (frames_px.h, cv_linear_px.h: compiled twice, written once), so a
// frame's bytes and a crop's bytes are the same whichever library produced them.
//
// Three kernels:
//   mixed_swap_kernel   rotation 0.  A maximal run of back-to-back frames is ONE run of pixels: nothing in the exchange depends on where
//                       a frame ends.  A run whose source and destination addresses agree mod 4 is `head` pixels byte by byte up to
//                       the first dword boundary that is also a pixel boundary (pixel k of a run at address a starts at a + 3k, and
//                       a + 3k = 0 (mod 4) for k = a mod 4), then 12-byte units of 4 pixels (one 12-byte load, the permute in
//                       registers, one 12-byte store), then at most 3 tail pixels byte by byte; any other run goes byte by byte.  A
//                       lane writes exactly the bytes it read, so the buffer may be its own destination.
//   mixed_turn_kernel   rotations 90 and 270.  turn_kernel's tile (frames.hip): 64 x 64 pixels through LDS stored transposed, rows of
//                       68 dwords, reads along source rows, writes along destination rows.  A workgroup finds its frame by a binary
//                       search of the per-frame first_block prefix the host built from the table, and takes the 12-byte path or the
//                       byte path per side from that frame's flags: wave-uniform, decided on the host from the frame's address
//                       (pointer + offset) and its size.  Edge tiles are cut by predicates: no byte outside a frame's range is written.
//   mixed_crops_kernel  face_crops_kernel (album.hip) with the frame's offset and row length read from the table.
//
// All addresses are 64-bit (a buffer may pass 2^31 bytes); inside a frame 32 bits do (a frame is below 2^31 bytes).
//
// Shared with the other five libraries: no symbol (linked with -fvisibility=hidden; this library has its own error string).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "../../include/hsefr_mixed.h"

#include "lib_error.h"
#include "frames_px.h"
#include "cv_linear_px.h"      // (turns contraction off from here on; csrc/build.sh adds the flag too)

using namespace hsefr;

#define MIXED_REQUIRE HSEFR_LIB_REQUIRE
#define MIXED_HIP_CHECK(expr) HSEFR_LIB_HIP_CHECK(expr, HSEFR_MIXED_ERR_NOMEM, HSEFR_MIXED_ERR_HIP)

namespace {

// host scratch of a call (malloc, not std::vector: the library exports its four entries and nothing of the C++ runtime's templates)
template <typename T>
struct HostArray {
    T* p;
    explicit HostArray(size_t n) : p((T*)malloc((n ? n : 1) * sizeof(T))) {}
    ~HostArray() { free(p); }
    HostArray(const HostArray&) = delete;
    HostArray& operator=(const HostArray&) = delete;
    T& operator[](size_t i) { return p[i]; }
};

constexpr int TILE = 64;                   // pixels per tile side
constexpr int TILE_STRIDE = TILE + 4;      // dwords per LDS row (frames.hip)
constexpr int THREADS = 256;
constexpr int SWAP_ITEMS = THREADS * 4;    // rotation 0: items (12-byte units or single pixels) of a run per workgroup
constexpr int UNITS_PER_BLOCK = 1024;      // crops: 16-byte pieces (or single bytes) of one face's output per workgroup
constexpr int MAX_TAPS = 4096;             // crops: oh + ow, the two tap tables of a workgroup in LDS (album.hip's limit)
constexpr int LOADV = 1, STOREV = 2;       // TurnFrame::flags

// what the kernels read of a frame (the device copy of the table, with what the host derived from it)
struct TurnFrame {                         // 32 bytes
    long long offset;
    int h, w;                              // the source size
    int first_block, tiles_x, flags, reserved;
};
struct SwapRun {                           // 32 bytes: a maximal run of back-to-back frames
    long long start;                       // byte offset of its first pixel
    long long items;                       // head + body + tail
    long long body;                        // 12-byte units behind the head
    int head, first_block;                 // pixels in front of the first unit
};
struct CropFrame {                         // hsefr_mixed_frame as the device reads it
    long long offset;
    int h, w;
};
static_assert(sizeof(TurnFrame) == 32 && sizeof(SwapRun) == 32 && sizeof(CropFrame) == sizeof(hsefr_mixed_frame), "table layout");

// the last row whose first_block is at most `block` (first_block ascends from 0; every row has at least one workgroup)
template <typename Row>
__device__ __forceinline__ int row_of_block(const Row* __restrict__ table, int n, int block) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (table[mid].first_block <= block)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// rotation 0.  src and dst may be the same buffer (no __restrict__): a lane reads its item before it writes it and no other lane
// touches it
__global__ __launch_bounds__(THREADS) void mixed_swap_kernel(const unsigned char* src, unsigned char* dst, const SwapRun* __restrict__ runs,
                                                             int n_runs, int swap) {
    const SwapRun run = runs[row_of_block(runs, n_runs, (int)blockIdx.x)];
    const long long first = (long long)((int)blockIdx.x - run.first_block) * SWAP_ITEMS;
    const long long last = min(first + SWAP_ITEMS, run.items);
    const long long head = run.head, vec_end = head + run.body;
    for (long long u = first + threadIdx.x; u < last; u += THREADS) {
        if (u >= head && u < vec_end) {
            const long long at = run.start + head * 3 + (u - head) * 12;
            unsigned p[4];
            unpack4(*reinterpret_cast<const Px4*>(src + at), swap != 0, p);
            store_px4(dst + at, pack4(p[0], p[1], p[2], p[3]));
        } else {
            const long long px = u < head ? u : head + run.body * 4 + (u - vec_end);
            const long long at = run.start + px * 3;
            store_pixel(dst + at, load_pixel(src + at, swap != 0));
        }
    }
}

// rotations 90 (ccw == 0: dst[x][h - 1 - y] = src[y][x]) and 270 (ccw != 0: dst[w - 1 - x][y] = src[y][x]); a frame's destination is
// [w, h, 3] at its own offset.  LOADV: the frame's source address 4-byte aligned and w a multiple of 4 (every source row starts on a
// dword, a tile's width is a multiple of 4 pixels); STOREV: its destination address 4-byte aligned and h a multiple of 4.
__global__ __launch_bounds__(THREADS) void mixed_turn_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                             const TurnFrame* __restrict__ table, int n, int ccw, int swap) {
    __shared__ __attribute__((aligned(16))) unsigned tile[TILE * TILE_STRIDE];      // tile[source column][source row]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const TurnFrame fr = table[row_of_block(table, n, (int)blockIdx.x)];
    const int h = fr.h, w = fr.w, tiles_x = fr.tiles_x;
    const int t = (int)blockIdx.x - fr.first_block;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int x0 = tx * TILE, y0 = ty * TILE;
    const int tw = min(TILE, w - x0), th = min(TILE, h - y0);                        // the tile's extent in the source: columns, rows
    const unsigned char* s = src + fr.offset;
    unsigned char* d = dst + fr.offset;
    if (fr.flags & LOADV) {
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
    if (fr.flags & STOREV) {
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
}

// VEC: a thread writes 16 consecutive bytes of its face's [oh, ow, 3] output with one store (the face's byte count is a multiple of 16
// and `out` is 16-byte aligned); otherwise one byte per thread.  album.hip's kernel, with the box's frame looked up in the table.
template <bool VEC>
__global__ __launch_bounds__(256) void mixed_crops_kernel(const unsigned char* __restrict__ frames, const CropFrame* __restrict__ table,
                                                          const int* __restrict__ boxes, unsigned char* __restrict__ out, int oh, int ow,
                                                          int units, int blocks_per_face) {
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
    const int bx = box[1], by = box[2], bw = box[3] - box[1], bh = box[4] - box[2];
    const CropFrame fr = table[box[0]];
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
    const long long wrow = (long long)fr.w * 3;
    const int rowb = ow * 3;
    const unsigned char* src = frames + fr.offset + by * wrow + (long long)bx * 3;
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

// ---- the host side -------------------------------------------------------------------------------------------------------------------
// The table's rules (hsefr_mixed.h).  `order`: the rows sorted by offset, for a caller that wants the runs.
int check_table(const char* who, const hsefr_mixed_frame* frames, int n_frames, long long buffer_bytes, int* order) {
    for (int i = 0; i < n_frames; ++i) {
        const hsefr_mixed_frame& f = frames[i];
        MIXED_REQUIRE(f.offset >= 0, HSEFR_MIXED_ERR_INVALID, "%s: frame %d at offset %lld", who, i, (long long)f.offset);
        MIXED_REQUIRE(f.h >= 1 && f.w >= 1, HSEFR_MIXED_ERR_INVALID, "%s: frame %d: bad frame size %d x %d", who, i, f.h, f.w);
        const long long bytes = (long long)f.h * f.w * 3;
        MIXED_REQUIRE(bytes < (1ll << 31), HSEFR_MIXED_ERR_UNSUPPORTED, "%s: frame %d of %d x %d is too large (2^31 bytes or more)", who, i, f.h,
                      f.w);
        MIXED_REQUIRE(f.offset <= buffer_bytes - bytes, HSEFR_MIXED_ERR_INVALID,
                      "%s: frame %d (%d x %d at offset %lld) ends past the buffer of %lld bytes", who, i, f.h, f.w, (long long)f.offset,
                      buffer_bytes);
    }
    for (int i = 0; i < n_frames; ++i) order[i] = i;
    std::sort(order, order + n_frames, [&](int a, int b) { return frames[a].offset < frames[b].offset; });
    for (int k = 1; k < n_frames; ++k) {
        const hsefr_mixed_frame &a = frames[order[k - 1]], &b = frames[order[k]];
        MIXED_REQUIRE(a.offset + (long long)a.h * a.w * 3 <= b.offset, HSEFR_MIXED_ERR_INVALID,
                      "%s: frames %d (%d x %d at offset %lld) and %d (at offset %lld) overlap", who, order[k - 1], a.h, a.w,
                      (long long)a.offset, order[k], (long long)b.offset);
    }
    return HSEFR_MIXED_OK;
}

// `bytes` of host memory on the device for one launch: allocation, copy, launch and release all in stream order
template <typename Launch>
int with_device_copy(const char* who, const void* host, size_t bytes, hipStream_t s, Launch launch) {
    void* d_table = nullptr;
    MIXED_HIP_CHECK(hipMallocAsync(&d_table, bytes, s));
    hipError_t e = hipMemcpyAsync(d_table, host, bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        launch(d_table);
        e = hipGetLastError();
    }
    const hipError_t e_free = hipFreeAsync(d_table, s);
    if (e == hipSuccess) e = e_free;
    if (e != hipSuccess) {
        set_error("%s: %s", who, hipGetErrorString(e));
        return HSEFR_MIXED_ERR_HIP;
    }
    return HSEFR_MIXED_OK;
}

int frames_prepare(const uint8_t* d_src, uint8_t* d_dst, long long buffer_bytes, const hsefr_mixed_frame* frames, int n_frames, int rotation,
                   int swap_rb, hipStream_t s) {
    MIXED_REQUIRE(rotation == 0 || rotation == 90 || rotation == 270, HSEFR_MIXED_ERR_INVALID, "frames_prepare: rotation %d (0, 90 or 270)",
                  rotation);
    MIXED_REQUIRE(n_frames >= 0 && buffer_bytes >= 0, HSEFR_MIXED_ERR_INVALID, "frames_prepare: negative size (n_frames = %d, buffer_bytes = %lld)",
                  n_frames, buffer_bytes);
    if (n_frames == 0) return HSEFR_MIXED_OK;
    MIXED_REQUIRE(d_src && d_dst && frames, HSEFR_MIXED_ERR_INVALID, "frames_prepare: null %s pointer with n_frames = %d",
                  !d_src ? "source" : (!d_dst ? "destination" : "table"), n_frames);
    MIXED_REQUIRE(rotation == 0 || d_dst != d_src, HSEFR_MIXED_ERR_INVALID, "frames_prepare: a quarter turn cannot run in place (rotation %d)",
                  rotation);
    HostArray<int> order((size_t)n_frames);
    HostArray<unsigned char> rows((size_t)n_frames * 32);      // the device table: SwapRun or TurnFrame rows
    MIXED_REQUIRE(order.p && rows.p, HSEFR_MIXED_ERR_NOMEM, "frames_prepare: out of host memory for the table of %d frames", n_frames);
    const int rc = check_table("frames_prepare", frames, n_frames, buffer_bytes, order.p);
    if (rc != HSEFR_MIXED_OK) return rc;
    const uintptr_t src_at = (uintptr_t)d_src, dst_at = (uintptr_t)d_dst;
    const dim3 block(THREADS);
    if (rotation == 0) {
        SwapRun* runs = (SwapRun*)rows.p;
        int n_runs = 0;
        long long blocks = 0;
        for (int k = 0; k < n_frames;) {
            const long long start = frames[order[k]].offset;
            long long end = start;
            for (; k < n_frames && frames[order[k]].offset == end; ++k)
                end += (long long)frames[order[k]].h * frames[order[k]].w * 3;
            const long long pixels = (end - start) / 3;
            SwapRun r;
            r.start = start;
            if (((src_at + (uintptr_t)start) & 3) == ((dst_at + (uintptr_t)start) & 3)) {
                const long long head = (long long)((src_at + (uintptr_t)start) & 3);      // see the head of the file
                r.head = (int)(head < pixels ? head : pixels);
                r.body = (pixels - r.head) / 4;
                r.items = r.head + r.body + (pixels - r.head) % 4;
            } else {
                MIXED_REQUIRE(pixels < (1ll << 31), HSEFR_MIXED_ERR_UNSUPPORTED,
                              "frames_prepare: a run of %lld pixels whose source and destination differ mod 4 is too long", pixels);
                r.head = (int)pixels;
                r.body = 0;
                r.items = pixels;
            }
            r.first_block = (int)blocks;
            blocks += (r.items + SWAP_ITEMS - 1) / SWAP_ITEMS;
            MIXED_REQUIRE(blocks < (1ll << 31), HSEFR_MIXED_ERR_UNSUPPORTED, "frames_prepare: %lld workgroups: too many", blocks);
            runs[n_runs++] = r;
        }
        return with_device_copy("frames_prepare", runs, (size_t)n_runs * sizeof(SwapRun), s, [&](void* d_table) {
            hipLaunchKernelGGL(mixed_swap_kernel, dim3((unsigned)blocks), block, 0, s, d_src, d_dst, (const SwapRun*)d_table, n_runs, swap_rb);
        });
    }
    TurnFrame* table = (TurnFrame*)rows.p;
    long long blocks = 0;
    for (int i = 0; i < n_frames; ++i) {
        const hsefr_mixed_frame& f = frames[i];
        TurnFrame& t = table[i];
        t.offset = f.offset;
        t.h = f.h;
        t.w = f.w;
        t.tiles_x = (f.w + TILE - 1) / TILE;
        t.first_block = (int)blocks;
        t.flags = ((((src_at + (uintptr_t)f.offset) & 3) == 0 && f.w % 4 == 0) ? LOADV : 0) |
                  ((((dst_at + (uintptr_t)f.offset) & 3) == 0 && f.h % 4 == 0) ? STOREV : 0);
        t.reserved = 0;
        blocks += (long long)t.tiles_x * ((f.h + TILE - 1) / TILE);
        MIXED_REQUIRE(blocks < (1ll << 31), HSEFR_MIXED_ERR_UNSUPPORTED, "frames_prepare: %lld tiles: too many", blocks);
    }
    const int ccw = rotation == 270;
    return with_device_copy("frames_prepare", table, (size_t)n_frames * sizeof(TurnFrame), s, [&](void* d_table) {
        hipLaunchKernelGGL(mixed_turn_kernel, dim3((unsigned)blocks), block, 0, s, d_src, d_dst, (const TurnFrame*)d_table, n_frames, ccw, swap_rb);
    });
}

int face_crops(const uint8_t* d_frames, long long buffer_bytes, const hsefr_mixed_frame* frames, int n_frames, const int32_t* boxes, int m,
               uint8_t* d_out, int oh, int ow, hipStream_t s) {
    MIXED_REQUIRE(m >= 0, HSEFR_MIXED_ERR_INVALID, "face_crops: m = %d", m);
    if (m == 0) return HSEFR_MIXED_OK;
    MIXED_REQUIRE(n_frames >= 0 && buffer_bytes >= 0, HSEFR_MIXED_ERR_INVALID, "face_crops: negative size (n_frames = %d, buffer_bytes = %lld)",
                  n_frames, buffer_bytes);
    MIXED_REQUIRE(d_frames && boxes && d_out && (frames || n_frames == 0), HSEFR_MIXED_ERR_INVALID, "face_crops: null %s pointer with m = %d",
                  !d_frames ? "frames" : (!boxes ? "boxes" : (!d_out ? "out" : "table")), m);
    MIXED_REQUIRE(oh > 0 && ow > 0, HSEFR_MIXED_ERR_INVALID, "face_crops: bad output size %d x %d", oh, ow);
    // one upload: the frame table, then the boxes (16-byte rows in front: both parts aligned)
    const size_t table_bytes = (size_t)n_frames * sizeof(CropFrame), box_bytes = (size_t)m * 5 * sizeof(int);
    HostArray<int> order((size_t)n_frames);
    HostArray<unsigned char> staged(table_bytes + box_bytes);
    MIXED_REQUIRE(order.p && staged.p, HSEFR_MIXED_ERR_NOMEM, "face_crops: out of host memory for the tables of %d frames and %d boxes", n_frames, m);
    const int rc = check_table("face_crops", frames, n_frames, buffer_bytes, order.p);
    if (rc != HSEFR_MIXED_OK) return rc;
    for (int i = 0; i < m; ++i) {
        const int32_t* b = boxes + (size_t)i * 5;
        MIXED_REQUIRE(b[0] >= 0 && b[0] < n_frames, HSEFR_MIXED_ERR_INVALID, "face_crops: box %d names frame %d of %d", i, b[0], n_frames);
        MIXED_REQUIRE(b[3] > b[1] && b[4] > b[2], HSEFR_MIXED_ERR_INVALID, "face_crops: box %d is empty (x %d..%d, y %d..%d)", i, b[1], b[3],
                      b[2], b[4]);
        const hsefr_mixed_frame& f = frames[b[0]];
        MIXED_REQUIRE(b[1] >= 0 && b[2] >= 0 && b[3] <= f.w && b[4] <= f.h, HSEFR_MIXED_ERR_INVALID,
                      "face_crops: box %d (x %d..%d, y %d..%d) is outside the %d x %d frame %d", i, b[1], b[3], b[2], b[4], f.w, f.h, b[0]);
    }
    MIXED_REQUIRE(oh + ow <= MAX_TAPS, HSEFR_MIXED_ERR_UNSUPPORTED, "face_crops: output %d x %d (the tap tables hold %d entries)", oh, ow, MAX_TAPS);
    const long long face_bytes = (long long)oh * ow * 3;
    MIXED_REQUIRE(face_bytes < (1ll << 31), HSEFR_MIXED_ERR_UNSUPPORTED, "face_crops: output %d x %d too large", oh, ow);
    const bool vec = face_bytes % 16 == 0 && ((uintptr_t)d_out & 15) == 0;
    const int units = (int)(vec ? face_bytes / 16 : face_bytes);
    const int blocks_per_face = (units + UNITS_PER_BLOCK - 1) / UNITS_PER_BLOCK;
    MIXED_REQUIRE((long long)m * blocks_per_face < (1ll << 31), HSEFR_MIXED_ERR_UNSUPPORTED, "face_crops: %d faces of %d x %d: too many", m, oh, ow);
    if (table_bytes) memcpy(staged.p, frames, table_bytes);
    memcpy(staged.p + table_bytes, boxes, box_bytes);
    const dim3 grid((unsigned)((long long)m * blocks_per_face)), block(256);
    const size_t lds = (size_t)(oh + ow) * 3 * sizeof(int);
    return with_device_copy("face_crops", staged.p, table_bytes + box_bytes, s, [&](void* d_table) {
        const CropFrame* d_frames_table = (const CropFrame*)d_table;
        const int* d_boxes = (const int*)((const unsigned char*)d_table + table_bytes);
        if (vec)
            hipLaunchKernelGGL(mixed_crops_kernel<true>, grid, block, lds, s, d_frames, d_frames_table, d_boxes, d_out, oh, ow, units, blocks_per_face);
        else
            hipLaunchKernelGGL(mixed_crops_kernel<false>, grid, block, lds, s, d_frames, d_frames_table, d_boxes, d_out, oh, ow, units, blocks_per_face);
    });
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int hsefr_mixed_version(void) { return HSEFR_MIXED_VERSION; }

__attribute__((visibility("default"))) const char* hsefr_mixed_last_error_string(void) { return g_error; }

__attribute__((visibility("default"))) int hsefr_mixed_frames_prepare(const uint8_t* d_src, uint8_t* d_dst, int64_t buffer_bytes,
                                                                       const hsefr_mixed_frame* frames, int n_frames, int rotation, int swap_rb,
                                                                       void* stream) {
    return frames_prepare(d_src, d_dst, (long long)buffer_bytes, frames, n_frames, rotation, swap_rb, (hipStream_t)stream);
}

__attribute__((visibility("default"))) int hsefr_mixed_face_crops(const uint8_t* d_frames, int64_t buffer_bytes, const hsefr_mixed_frame* frames,
                                                                   int n_frames, const int32_t* boxes, int m, uint8_t* d_out, int oh, int ow,
                                                                   void* stream) {
    return face_crops(d_frames, (long long)buffer_bytes, frames, n_frames, boxes, m, d_out, oh, ow, (hipStream_t)stream);
}

}  // extern "C"
