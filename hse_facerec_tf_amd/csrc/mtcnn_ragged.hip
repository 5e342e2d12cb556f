// libhsefr_ragged.so (include/hsefr_ragged.h): one MTCNN detector pass over frames of different sizes.
//
// The same-size pass (hsefr.h's *_batch entries) takes a frame as a grid index and the sizes as scalars; here a pass is one list of
// (frame, pyramid level) items with their own dimensions and 64-bit offsets in packed buffers, and a launch covers the whole list.
// An item's threads are padded to whole workgroups of 256, and a workgroup reads its item from the plan's workgroup -> item table
// once (a few hundred items at most): no launch per item or per level.
//
// Why the bits are the single-frame bits:
//   - the pyramid, the crops and the box logic call the one-frame bodies of area_resize_px.h and mtcnn_post_frame.h, the code
//     libhsefr.so compiles, with the item's or the frame's pointers and sizes read from a table instead of derived from blockIdx;
//   - the convolution gives a thread CO consecutive output channels of one output pixel and runs each output's FMA chain kh, kw, c
//     ascending from the bias with fmaf -- conv2d_direct_kernel's order (smallnet.hip), which does not depend on CO or on how many
//     input channels one load brings; the pooling takes fmaxf over the window clipped to the item in maxpool_f32_kernel's order.
// The tables come from the device, so the host cannot check them: every kernel checks an item against the counts and buffer sizes
// passed with the tables and skips what does not fit (workgroup-uniform, before any access).
//
// Plain fp32 VALU kernels as smallnet.hip's: P-Net's channel counts (3 / 10 / 16 / 32) are not MFMA shapes and a pass is launch-bound.
//
// Shared with the other four libraries: nothing at link time (-fvisibility=hidden; this library has its own error string).
#include <hip/hip_runtime.h>

#include "../../include/hsefr_ragged.h"
#include "area_resize_px.h"
#include "lib_error.h"
#include "mtcnn_post_frame.h"

#define RAGGED_REQUIRE HSEFR_LIB_REQUIRE

namespace hsefr {

namespace {

int launch_status(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("launch of %s failed: %s", what, hipGetErrorString(e));
        return HSEFR_RAGGED_ERR_HIP;
    }
    return HSEFR_RAGGED_OK;
}

constexpr int THREADS = 256;
constexpr int MAX_LEVEL_LDS = 64 * 1024;      // the row form's bound in area_resize.hip

// the frame's bytes lie inside the packed buffer
__device__ __forceinline__ bool frame_inside(const hsefr_ragged_frame& f, long long frames_bytes) {
    return f.h > 0 && f.w > 0 && f.offset >= 0 && (long long)f.h * f.w * 3 < (1ll << 31) && f.offset + (long long)f.h * f.w * 3 <= frames_bytes;
}

// the workgroup's item, or -1 (a table that points outside the list)
__device__ __forceinline__ int block_item_of(const int* __restrict__ block_item, int n_items) {
    const int it = block_item[blockIdx.x];
    return it >= 0 && it < n_items ? it : -1;
}

// ---- the pyramid: a workgroup is a destination row (rows != 0) or 256 destination pixels of its item ------------------------------
__global__ __launch_bounds__(THREADS) void ragged_pyramid_kernel(const unsigned char* __restrict__ frames, long long frames_bytes,
                                                                 const hsefr_ragged_frame* __restrict__ frame_tab, int n_frames,
                                                                 const hsefr_ragged_level* __restrict__ items, int n_items,
                                                                 const int* __restrict__ block_item, float* __restrict__ levels,
                                                                 long long levels_elems, int lds_bytes) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int it = block_item_of(block_item, n_items);
    if (it < 0) return;
    const hsefr_ragged_level m = items[it];
    if (m.frame < 0 || m.frame >= n_frames || m.dh <= 0 || m.dw <= 0 || m.level_off < 0 || (long long)m.dh * m.dw * 3 >= (1ll << 31) ||
        m.level_off + (long long)m.dh * m.dw * 3 > levels_elems)
        return;
    const hsefr_ragged_frame f = frame_tab[m.frame];
    if (!frame_inside(f, frames_bytes)) return;
    const int local = (int)blockIdx.x - m.first_block;
    if (local < 0) return;
    const unsigned char* src = frames + f.offset;
    float* dst = levels + m.level_off;
    if (m.rows) {
        // the row form reads only a decimated frame (both factors >= 1) and needs its LDS: what the plan promises is checked here
        const double fy = (double)f.h / m.dh;
        const long long need = (long long)m.hoff + ((long long)fy + 3) * m.dw * 3 * (long long)sizeof(float);
        if (local >= m.dh || f.h < m.dh || f.w < m.dw || m.hoff < (int)(m.dw * sizeof(XCell)) || (m.hoff & 15) || need > lds_bytes) return;
        area_level_row(src, dst, f.h, f.w, m.dh, m.dw, m.hoff, local, lds);
    } else {
        const long long i = (long long)local * THREADS + threadIdx.x;
        if (i >= (long long)m.dh * m.dw) return;
        area_level_pixel(src, dst, f.h, f.w, m.dh, m.dw, (int)i);
    }
}

// ---- a P-Net convolution over the item list (stride 1, VALID) ----------------------------------------------------------------------
// Thread = CO consecutive output channels of one output pixel of the workgroup's item; conv2d_direct_kernel's loads and FMA order.
template <int CO>
__global__ __launch_bounds__(THREADS) void ragged_conv2d_kernel(const float* __restrict__ x, long long x_pixels, const float* __restrict__ w,
                                                                const float* __restrict__ bias, const float* __restrict__ alpha,
                                                                float* __restrict__ y, long long y_pixels,
                                                                const hsefr_ragged_map* __restrict__ maps, int n_items,
                                                                const int* __restrict__ block_item, int C, int Cout, int KH, int KW) {
    typedef float vco __attribute__((ext_vector_type(CO == 1 ? 2 : CO)));      // (CO == 1 reads scalars; the type is unused then)
    const int it = block_item_of(block_item, n_items);
    if (it < 0) return;
    const hsefr_ragged_map m = maps[it];
    const int local = (int)blockIdx.x - m.first_block;
    if (local < 0 || m.ih <= 0 || m.iw <= 0 || m.oh <= 0 || m.ow <= 0 || m.oh > m.ih - KH + 1 || m.ow > m.iw - KW + 1 || m.in_off < 0 ||
        m.out_off < 0 || (long long)m.ih * m.iw * C >= (1ll << 31) || m.in_off + (long long)m.ih * m.iw > x_pixels ||
        m.out_off + (long long)m.oh * m.ow > y_pixels)
        return;
    const int cg = Cout / CO;
    const long long i = (long long)local * THREADS + threadIdx.x;              // index over the item's pixels x (Cout / CO)
    if (i >= (long long)m.oh * m.ow * cg) return;
    const int co = (int)(i % cg) * CO;
    const int p = (int)(i / cg);
    const int ow = p % m.ow, oh = p / m.ow;
    float acc[CO];
#pragma unroll
    for (int j = 0; j < CO; ++j) acc[j] = bias ? bias[co + j] : 0.f;
    const float* xn = x + m.in_off * C;
    // what the ALIGNMENT of the item's first pixel allows (a pixel row is C floats, so C % 4 == 0 keeps every pixel as aligned)
    const int xvec = ((uintptr_t)xn & 15) == 0 ? 4 : (((uintptr_t)xn & 7) == 0 ? 2 : 1);
    auto wld = [&](const float* q, float* out) __attribute__((always_inline)) {
        if constexpr (CO == 1) out[0] = q[0];
        else {
            const vco v = *(const vco*)q;
#pragma unroll
            for (int j = 0; j < CO; ++j) out[j] = v[j];
        }
    };
    for (int kh = 0; kh < KH; ++kh) {
        for (int kw = 0; kw < KW; ++kw) {
            const float* xp = xn + ((long long)(oh + kh) * m.iw + ow + kw) * C;
            const float* wp = w + (long long)((kh * KW + kw) * C) * Cout + co;
            int c = 0;
            if (xvec >= 4 && (C & 3) == 0) {
                for (; c < C; c += 4) {
                    const float4 xv = *(const float4*)(xp + c);
                    float w0[CO], w1[CO], w2[CO], w3[CO];
                    wld(wp + (long long)c * Cout, w0); wld(wp + (long long)(c + 1) * Cout, w1);
                    wld(wp + (long long)(c + 2) * Cout, w2); wld(wp + (long long)(c + 3) * Cout, w3);
#pragma unroll
                    for (int j = 0; j < CO; ++j) acc[j] = fmaf(xv.w, w3[j], fmaf(xv.z, w2[j], fmaf(xv.y, w1[j], fmaf(xv.x, w0[j], acc[j]))));
                }
            } else if (xvec >= 2 && (C & 1) == 0) {
                for (; c < C; c += 2) {
                    const float2 xv = *(const float2*)(xp + c);
                    float w0[CO], w1[CO];
                    wld(wp + (long long)c * Cout, w0); wld(wp + (long long)(c + 1) * Cout, w1);
#pragma unroll
                    for (int j = 0; j < CO; ++j) acc[j] = fmaf(xv.y, w1[j], fmaf(xv.x, w0[j], acc[j]));
                }
            }
            for (; c < C; ++c) {
                float w0[CO];
                wld(wp + (long long)c * Cout, w0);
#pragma unroll
                for (int j = 0; j < CO; ++j) acc[j] = fmaf(xp[c], w0[j], acc[j]);
            }
        }
    }
    float* yo = y + (m.out_off + p) * Cout + co;
#pragma unroll
    for (int j = 0; j < CO; ++j) {
        float a = acc[j];
        if (alpha) a = a > 0.f ? a : alpha[co + j] * a;
        yo[j] = a;
    }
}

// ---- max-pool k x k / stride, SAME: windows clipped to the item (== TF's -inf padding) ----------------------------------------------
__global__ __launch_bounds__(THREADS) void ragged_maxpool_kernel(const float* __restrict__ x, long long x_pixels, float* __restrict__ y,
                                                                 long long y_pixels, const hsefr_ragged_map* __restrict__ maps, int n_items,
                                                                 const int* __restrict__ block_item, int C, int K, int stride) {
    const int it = block_item_of(block_item, n_items);
    if (it < 0) return;
    const hsefr_ragged_map m = maps[it];
    const int local = (int)blockIdx.x - m.first_block;
    if (local < 0 || m.ih <= 0 || m.iw <= 0 || m.oh != (m.ih + stride - 1) / stride || m.ow != (m.iw + stride - 1) / stride || m.in_off < 0 ||
        m.out_off < 0 || (long long)m.ih * m.iw * C >= (1ll << 31) || m.in_off + (long long)m.ih * m.iw > x_pixels ||
        m.out_off + (long long)m.oh * m.ow > y_pixels)
        return;
    const long long i = (long long)local * THREADS + threadIdx.x;
    if (i >= (long long)m.oh * m.ow * C) return;
    const int c = (int)(i % C);
    const int p = (int)(i / C);
    const int ow = p % m.ow, oh = p / m.ow;
    // TF's SAME rule: the padding before is half of the total, rounded down
    const int tot_h = (m.oh - 1) * stride + K - m.ih, tot_w = (m.ow - 1) * stride + K - m.iw;
    const int pad_t = (tot_h > 0 ? tot_h : 0) / 2, pad_l = (tot_w > 0 ? tot_w : 0) / 2;
    const float* xn = x + m.in_off * C;
    float v = -INFINITY;
    for (int kh = 0; kh < K; ++kh) {
        const int ih = oh * stride - pad_t + kh;
        if (ih < 0 || ih >= m.ih) continue;
        for (int kw = 0; kw < K; ++kw) {
            const int iw = ow * stride - pad_l + kw;
            if (iw < 0 || iw >= m.iw) continue;
            v = fmaxf(v, xn[((long long)ih * m.iw + iw) * C + c]);
        }
    }
    y[(m.out_off + p) * C + c] = v;
}

// ---- stage 1: one workgroup per frame walks the frame's levels, then finishes ------------------------------------------------------
// A level's body leaves through early returns that are uniform over the workgroup, and the next level starts by resetting the LDS
// list the slowest thread may still be reading; it also reads the `counters` and `found` rows thread 0 and others wrote for the level
// before.  Hence the barrier after EVERY level (it orders the workgroup's global writes too), the last one in front of the finish.
__global__ __launch_bounds__(NT) void ragged_stage1_kernel(const float* __restrict__ prob, const float* __restrict__ reg, long long n_cells,
                                                           const hsefr_ragged_frame* __restrict__ frame_tab,
                                                           const hsefr_ragged_cells* __restrict__ cells, int n_items, float thr,
                                                           double* __restrict__ found, int* __restrict__ counters, double* __restrict__ boxes,
                                                           int* __restrict__ tab) {
    const size_t b = blockIdx.x;
    const hsefr_ragged_frame f = frame_tab[b];
    double* fnd = found + b * CAP * 9;
    int* cnt = counters + b * 8;
    int n = f.n_items;
    if (f.first_item < 0 || n < 0 || (long long)f.first_item + n > n_items) n = 0;       // a range outside the list: no level
    for (int k = 0; k < n; ++k) {
        const hsefr_ragged_cells c = cells[f.first_item + k];
        const bool inside = c.w > 0 && c.h > 0 && c.scale > 0 && (long long)c.w * c.h < (1ll << 31) && c.cell_off >= 0 &&
                            c.cell_off + (long long)c.w * c.h <= n_cells;
        if (inside) stage1_level_frame(prob + c.cell_off * 2, reg + c.cell_off * 4, c.w, c.h, c.scale, thr, fnd, cnt);
        __syncthreads();
    }
    stage1_finish_frame(fnd, cnt, boxes + b * CAP * 5, tab + b * CAP * 8, f.w, f.h);
}

// ---- the crops of all frames as one list: area_crops_kernel's batched form with the frame from the table -----------------------------
__global__ __launch_bounds__(THREADS) void ragged_crops_kernel(const unsigned char* __restrict__ frames, long long frames_bytes,
                                                               const hsefr_ragged_frame* __restrict__ frame_tab, const int* __restrict__ tables,
                                                               const int* __restrict__ offsets, float* __restrict__ dst, int B, int rows, int n,
                                                               int S) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= (long long)n * S * S) return;
    const int k = (int)(i / (S * S)), rem = (int)(i - (long long)k * S * S), dy = rem / S, dx = rem - dy * S;
    int lo = 0, hi = B;                                                       // the last b with offsets[b] <= k
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= k) lo = mid; else hi = mid;
    }
    const int row = k - offsets[lo];
    if (row < 0 || row >= rows || k >= offsets[lo + 1]) return;
    const hsefr_ragged_frame f = frame_tab[lo];
    if (!frame_inside(f, frames_bytes)) return;
    area_crop_pixel(frames + f.offset, tables + ((size_t)lo * rows + row) * 8, dst + (((long long)k * S + dx) * S + dy) * 3, f.w, S, dy, dx);
}

// ---- stage 2 / 3 of all frames: stage23_finish_kernel's batched form with img_w, img_h from the table ------------------------------
template <int STAGE>
__global__ __launch_bounds__(NT) void ragged_stage23_kernel(const double* __restrict__ boxes_in, const int* __restrict__ offsets /*[B+1]*/,
                                                            int n_total, const float* __restrict__ prob, const float* __restrict__ reg,
                                                            const float* __restrict__ pts, float thr, double* __restrict__ boxes_out,
                                                            int* __restrict__ tab_out, float* __restrict__ points_out, int* __restrict__ counters,
                                                            const hsefr_ragged_frame* __restrict__ frame_tab) {
    const size_t b = blockIdx.x;
    const int lo = offsets[b], hi = offsets[b + 1];
    const bool inside = lo >= 0 && lo <= hi && hi <= n_total;
    const size_t first = inside ? (size_t)lo : 0;
    const int n = inside ? hi - lo : CAP + 1;
    const hsefr_ragged_frame f = frame_tab[b];
    stage23_finish_frame<STAGE>(boxes_in + b * CAP * 5, n, prob + first * 2, reg + first * 4, STAGE == 3 ? pts + first * 10 : nullptr, thr,
                                boxes_out + b * CAP * 5, STAGE == 2 ? tab_out + b * CAP * 8 : nullptr,
                                STAGE == 3 ? points_out + b * CAP * 10 : nullptr, counters + b * 8, f.w, f.h);
}

template <class K>
int set_lds(K kernel) {
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PostLds));
    if (e != hipSuccess) {
        set_error("hipFuncSetAttribute failed: %s", hipGetErrorString(e));
        return HSEFR_RAGGED_ERR_HIP;
    }
    return HSEFR_RAGGED_OK;
}

}  // namespace

}  // namespace hsefr

using namespace hsefr;

#define RAGGED_API extern "C" __attribute__((visibility("default")))

RAGGED_API int hsefr_ragged_version(void) { return HSEFR_RAGGED_VERSION; }

RAGGED_API const char* hsefr_ragged_last_error_string(void) { return g_error; }

RAGGED_API int hsefr_ragged_capacity(void) { return CAP; }

RAGGED_API int hsefr_ragged_pyramid(const uint8_t* d_frames, int64_t frames_bytes, const hsefr_ragged_frame* d_frame_tab, int n_frames,
                                    const hsefr_ragged_level* d_items, int n_items, const int32_t* d_block_item, int n_blocks, float* d_levels,
                                    int64_t levels_elems, int lds_bytes, void* stream) {
    RAGGED_REQUIRE(n_frames >= 0 && n_items >= 0 && n_blocks >= 0 && frames_bytes >= 0 && levels_elems >= 0, HSEFR_RAGGED_ERR_INVALID,
                   "pyramid: negative size (%d frames, %d items, %d workgroups, %lld bytes, %lld floats)", n_frames, n_items, n_blocks,
                   (long long)frames_bytes, (long long)levels_elems);
    RAGGED_REQUIRE(lds_bytes >= 0 && lds_bytes <= MAX_LEVEL_LDS, HSEFR_RAGGED_ERR_INVALID, "pyramid: %d bytes of LDS (0 .. %d)", lds_bytes,
                   MAX_LEVEL_LDS);
    if (n_items == 0 || n_blocks == 0 || n_frames == 0) return HSEFR_RAGGED_OK;
    RAGGED_REQUIRE(d_frame_tab && d_items && d_block_item, HSEFR_RAGGED_ERR_INVALID, "pyramid: null table with %d items", n_items);
    RAGGED_REQUIRE(d_frames && d_levels, HSEFR_RAGGED_ERR_INVALID, "pyramid: null %s pointer with %d items", !d_frames ? "frame" : "level", n_items);
    hipLaunchKernelGGL(ragged_pyramid_kernel, dim3((unsigned)n_blocks), dim3(THREADS), (size_t)lds_bytes, (hipStream_t)stream, d_frames,
                       (long long)frames_bytes, d_frame_tab, n_frames, d_items, n_items, d_block_item, d_levels, (long long)levels_elems, lds_bytes);
    return launch_status("ragged_pyramid");
}

RAGGED_API int hsefr_ragged_conv2d(const float* x, int64_t x_pixels, const float* w, const float* bias, const float* alpha, float* y,
                                   int64_t y_pixels, const hsefr_ragged_map* d_maps, int n_items, const int32_t* d_block_item, int n_blocks, int c,
                                   int cout, int kh, int kw, int stride, int pad_t, int pad_l, int co, void* stream) {
    RAGGED_REQUIRE(n_items >= 0 && n_blocks >= 0 && x_pixels >= 0 && y_pixels >= 0, HSEFR_RAGGED_ERR_INVALID,
                   "conv2d: negative size (%d items, %d workgroups, %lld / %lld pixels)", n_items, n_blocks, (long long)x_pixels, (long long)y_pixels);
    RAGGED_REQUIRE(c > 0 && cout > 0 && kh > 0 && kw > 0 && stride > 0, HSEFR_RAGGED_ERR_INVALID, "conv2d: bad shape (c %d, cout %d, kernel %dx%d, stride %d)",
                   c, cout, kh, kw, stride);
    RAGGED_REQUIRE(stride == 1 && pad_t == 0 && pad_l == 0, HSEFR_RAGGED_ERR_UNSUPPORTED,
                   "conv2d: stride %d with padding %d, %d is not supported (stride 1, VALID)", stride, pad_t, pad_l);
    RAGGED_REQUIRE((co == 1 || co == 2 || co == 4) && cout % co == 0, HSEFR_RAGGED_ERR_INVALID, "conv2d: co = %d with cout = %d (1, 2 or 4, a divisor)",
                   co, cout);
    RAGGED_REQUIRE((long long)kh * kw * c * cout < (1ll << 31), HSEFR_RAGGED_ERR_UNSUPPORTED, "conv2d: a %dx%dx%dx%d kernel is too large", kh, kw, c, cout);
    if (n_items == 0 || n_blocks == 0) return HSEFR_RAGGED_OK;
    RAGGED_REQUIRE(d_maps && d_block_item, HSEFR_RAGGED_ERR_INVALID, "conv2d: null table with %d items", n_items);
    RAGGED_REQUIRE(x && w && y, HSEFR_RAGGED_ERR_INVALID, "conv2d: null %s pointer with %d items", !x ? "input" : (!w ? "weight" : "output"), n_items);
    RAGGED_REQUIRE(((uintptr_t)w & (size_t)(4 * co - 1)) == 0, HSEFR_RAGGED_ERR_INVALID, "conv2d: the weights are not aligned to %d bytes (co = %d)", 4 * co,
                   co);
#define RAGGED_CONV(CO)                                                                                                                      \
    hipLaunchKernelGGL(ragged_conv2d_kernel<CO>, dim3((unsigned)n_blocks), dim3(THREADS), 0, (hipStream_t)stream, x, (long long)x_pixels, w, bias, \
                       alpha, y, (long long)y_pixels, d_maps, n_items, d_block_item, c, cout, kh, kw)
    if (co == 4) RAGGED_CONV(4);
    else if (co == 2) RAGGED_CONV(2);
    else RAGGED_CONV(1);
#undef RAGGED_CONV
    return launch_status("ragged_conv2d");
}

RAGGED_API int hsefr_ragged_maxpool(const float* x, int64_t x_pixels, float* y, int64_t y_pixels, const hsefr_ragged_map* d_maps, int n_items,
                                    const int32_t* d_block_item, int n_blocks, int c, int k, int stride, void* stream) {
    RAGGED_REQUIRE(n_items >= 0 && n_blocks >= 0 && x_pixels >= 0 && y_pixels >= 0, HSEFR_RAGGED_ERR_INVALID,
                   "maxpool: negative size (%d items, %d workgroups, %lld / %lld pixels)", n_items, n_blocks, (long long)x_pixels, (long long)y_pixels);
    RAGGED_REQUIRE(c > 0 && k > 0 && stride > 0 && k < 32768 && stride < 32768, HSEFR_RAGGED_ERR_INVALID, "maxpool: bad shape (c %d, k %d, stride %d)", c, k,
                   stride);
    if (n_items == 0 || n_blocks == 0) return HSEFR_RAGGED_OK;
    RAGGED_REQUIRE(d_maps && d_block_item, HSEFR_RAGGED_ERR_INVALID, "maxpool: null table with %d items", n_items);
    RAGGED_REQUIRE(x && y, HSEFR_RAGGED_ERR_INVALID, "maxpool: null %s pointer with %d items", !x ? "input" : "output", n_items);
    hipLaunchKernelGGL(ragged_maxpool_kernel, dim3((unsigned)n_blocks), dim3(THREADS), 0, (hipStream_t)stream, x, (long long)x_pixels, y,
                       (long long)y_pixels, d_maps, n_items, d_block_item, c, k, stride);
    return launch_status("ragged_maxpool");
}

RAGGED_API int hsefr_ragged_stage1(const float* prob, const float* reg, int64_t n_cells, const hsefr_ragged_frame* d_frame_tab, int n_frames,
                                   const hsefr_ragged_cells* d_cells, int n_items, float thr, double* found, int32_t* counters, double* boxes,
                                   int32_t* tab, void* stream) {
    RAGGED_REQUIRE(n_frames >= 0 && n_items >= 0 && n_cells >= 0, HSEFR_RAGGED_ERR_INVALID, "stage1: negative size (%d frames, %d items, %lld cells)",
                   n_frames, n_items, (long long)n_cells);
    if (n_frames == 0) return HSEFR_RAGGED_OK;
    RAGGED_REQUIRE(d_frame_tab && (d_cells || n_items == 0), HSEFR_RAGGED_ERR_INVALID, "stage1: null table with %d frames, %d items", n_frames, n_items);
    RAGGED_REQUIRE((prob && reg) || n_items == 0, HSEFR_RAGGED_ERR_INVALID, "stage1: null map pointer with %d items", n_items);
    RAGGED_REQUIRE(found && counters && boxes && tab, HSEFR_RAGGED_ERR_INVALID, "stage1: null list pointer with %d frames", n_frames);
    if (int rc = set_lds(ragged_stage1_kernel)) return rc;
    hipLaunchKernelGGL(ragged_stage1_kernel, dim3((unsigned)n_frames), dim3(NT), sizeof(PostLds), (hipStream_t)stream, prob, reg, (long long)n_cells,
                       d_frame_tab, d_cells, n_items, thr, found, counters, boxes, tab);
    return launch_status("ragged_stage1");
}

RAGGED_API int hsefr_ragged_crops(const uint8_t* d_frames, int64_t frames_bytes, const hsefr_ragged_frame* d_frame_tab, int n_frames,
                                  const int32_t* tables, const int32_t* offsets, float* dst, int rows, int n, int size, void* stream) {
    RAGGED_REQUIRE(n_frames >= 0 && rows >= 0 && n >= 0 && size > 0 && frames_bytes >= 0, HSEFR_RAGGED_ERR_INVALID,
                   "crops: bad shape (%d frames, %d rows, %d crops of size %d, %lld bytes)", n_frames, rows, n, size, (long long)frames_bytes);
    // the kernel indexes the tables' rows and a crop's pixels with int
    RAGGED_REQUIRE((long long)n_frames * rows < (1ll << 31) && (long long)size * size < (1ll << 31), HSEFR_RAGGED_ERR_UNSUPPORTED,
                   "crops: %d frames with %d table rows, size %d: an index leaves 31 bits", n_frames, rows, size);
    if (n == 0 || n_frames == 0) return HSEFR_RAGGED_OK;
    const long long total = (long long)n * size * size;
    RAGGED_REQUIRE((total + THREADS - 1) / THREADS < (1ll << 31), HSEFR_RAGGED_ERR_UNSUPPORTED, "crops: %d crops of size %d", n, size);
    RAGGED_REQUIRE(d_frame_tab && tables && offsets, HSEFR_RAGGED_ERR_INVALID, "crops: null table with %d crops", n);
    RAGGED_REQUIRE(d_frames && dst, HSEFR_RAGGED_ERR_INVALID, "crops: null %s pointer with %d crops", !d_frames ? "frame" : "crop", n);
    hipLaunchKernelGGL(ragged_crops_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, d_frames,
                       (long long)frames_bytes, d_frame_tab, tables, offsets, dst, n_frames, rows, n, size);
    return launch_status("ragged_crops");
}

RAGGED_API int hsefr_ragged_stage_finish(int stage, const double* boxes_in, const int32_t* offsets, int n_total, const float* prob, const float* reg,
                                         const float* pts, float thr, double* boxes_out, int32_t* tab_out, float* points_out, int32_t* counters,
                                         const hsefr_ragged_frame* d_frame_tab, int n_frames, void* stream) {
    RAGGED_REQUIRE((stage == 2 || stage == 3) && n_frames >= 0 && n_total >= 0, HSEFR_RAGGED_ERR_INVALID, "stage_finish: stage %d, %d frames, %d rows", stage,
                   n_frames, n_total);
    if (n_frames == 0) return HSEFR_RAGGED_OK;
    RAGGED_REQUIRE(d_frame_tab && offsets, HSEFR_RAGGED_ERR_INVALID, "stage_finish: null table with %d frames", n_frames);
    RAGGED_REQUIRE(boxes_in && boxes_out && counters && (stage == 2 ? tab_out != nullptr : points_out != nullptr) &&
                       ((prob && reg && (stage == 2 || pts)) || n_total == 0),
                   HSEFR_RAGGED_ERR_INVALID, "stage_finish: null pointer at stage %d with %d frames, %d rows", stage, n_frames, n_total);
    if (stage == 2) {
        if (int rc = set_lds(ragged_stage23_kernel<2>)) return rc;
        hipLaunchKernelGGL(ragged_stage23_kernel<2>, dim3((unsigned)n_frames), dim3(NT), sizeof(PostLds), (hipStream_t)stream, boxes_in, offsets, n_total,
                           prob, reg, pts, thr, boxes_out, tab_out, points_out, counters, d_frame_tab);
    } else {
        if (int rc = set_lds(ragged_stage23_kernel<3>)) return rc;
        hipLaunchKernelGGL(ragged_stage23_kernel<3>, dim3((unsigned)n_frames), dim3(NT), sizeof(PostLds), (hipStream_t)stream, boxes_in, offsets, n_total,
                           prob, reg, pts, thr, boxes_out, tab_out, points_out, counters, d_frame_tab);
    }
    return launch_status("ragged_stage_finish");
}
