// MTCNN's box logic on the device: candidate generation from the P-Net maps, greedy NMS, box regression, squaring, the crop
// windows of the next stage and the landmark transform (generateBoundingBox / nms / bbreg / rerec / pad of
// facial_analysis.py:354-476, driven by mtcnn_detect_faces :478-604).  With the pyramid and the crops already resampled on the
// GPU (area_resize.hip) the cascade's host side shrinks to three 32-byte read-backs of box counts per frame.
//
// Parity contract: the SAME numbers as the host restatement in mtcnn.py (float64 box arithmetic, float32 scores / regressions /
// landmarks, products and sums rounded separately as NumPy does: every a + b * c below is written with __dmul_rn / __dadd_rn so
// that hipcc cannot contract it), the same greedy order: descending score, ties by DESCENDING candidate index (see make_key; for
// P-Net candidates the index is the row-major index of the cell in the [W', H'] map, which is the order np.nonzero yields).
//
// One workgroup of 1024 threads per call (a frame has a few hundred candidates per level): candidates are appended unordered
// with an LDS atomic, a bitonic sort of 64-bit keys (score | index) makes the order deterministic, the greedy pass walks the
// sorted list with one barrier per KEPT box.  More than MTCNN_CAP candidates in one list raise the overflow flag; the Python
// side then redoes that frame on its host path.
#include "common.h"
#include "mtcnn_post_frame.h"      // the one-frame bodies (shared with mtcnn_ragged.hip): PostLds, the sort, the NMS, stage1_level_frame, ...

namespace hsefr {

namespace {

// One workgroup per frame (blockIdx.x) over prob [B,w,h,2], reg [B,w,h,4], found [B,CAP,9], counters [B,8]; one frame is a grid of 1.
// Here and in the two entries below a frame's workgroup touches its own rows and its own counters only, overflow flag included: what
// a frame gets does not depend on its neighbours.  PostLds takes 108 KB of the CU's 160 KB, so the B workgroups spread one per CU.
// (One entry serves both the single-frame and the batched C functions: a second instantiation of each body would take the product
// library past the size tests/test_abi_cpu.py holds it to.)
__global__ __launch_bounds__(NT) void stage1_level_kernel(const float* __restrict__ prob, const float* __restrict__ reg, int w, int h, double scale,
                                                          float thr, double* __restrict__ found, int* __restrict__ counters) {
    const size_t b = blockIdx.x, cells = (size_t)w * h;
    stage1_level_frame(prob + b * cells * 2, reg + b * cells * 4, w, h, scale, thr, found + b * CAP * 9, counters + b * 8);
}

// found [B,CAP,9], counters [B,8] -> boxes [B,CAP,5], tab [B,CAP,8]
__global__ __launch_bounds__(NT) void stage1_finish_kernel(const double* __restrict__ found, int* __restrict__ counters, double* __restrict__ boxes,
                                                           int* __restrict__ tab, int img_w, int img_h) {
    const size_t b = blockIdx.x;
    stage1_finish_frame(found + b * CAP * 9, counters + b * 8, boxes + b * CAP * 5, tab + b * CAP * 8, img_w, img_h);
}

// offsets == nullptr: one frame, the nets ran on its n boxes.  Otherwise B frames with boxes_in / boxes_out [B,CAP,5], tab_out [B,CAP,8],
// points_out [B,CAP,10], counters [B,8], and the nets ran on the crops of all frames as one list of n_total rows: rows offsets[b] ..
// offsets[b + 1] of prob / reg / pts are frame b's, in the order of its boxes_in rows.  An empty range writes count 0; a range that is
// not inside the list is refused the way a list above the capacity is: flag, count 0, nothing read.
template <int STAGE>
__global__ __launch_bounds__(NT) void stage23_finish_kernel(const double* __restrict__ boxes_in, int n, const int* __restrict__ offsets /*[B+1]*/,
                                                            int n_total, const float* __restrict__ prob, const float* __restrict__ reg,
                                                            const float* __restrict__ pts, float thr, double* __restrict__ boxes_out,
                                                            int* __restrict__ tab_out, float* __restrict__ points_out, int* __restrict__ counters,
                                                            int img_w, int img_h) {
    const size_t b = blockIdx.x;
    size_t first = 0;
    if (offsets) {
        const int lo = offsets[b], hi = offsets[b + 1];
        const bool inside = lo >= 0 && lo <= hi && hi <= n_total;
        first = inside ? (size_t)lo : 0;
        n = inside ? hi - lo : CAP + 1;
    }
    stage23_finish_frame<STAGE>(boxes_in + b * CAP * 5, n, prob + first * 2, reg + first * 4, STAGE == 3 ? pts + first * 10 : nullptr, thr,
                                boxes_out + b * CAP * 5, STAGE == 2 ? tab_out + b * CAP * 8 : nullptr,
                                STAGE == 3 ? points_out + b * CAP * 10 : nullptr, counters + b * 8, img_w, img_h);
}

// a plain NMS over a box list, for the unit tests: keep[] = kept ORIGINAL indices in pick order, *n_keep their number
__global__ __launch_bounds__(NT) void nms_kernel(const double* __restrict__ boxes /*[n,5]*/, int n, double thr, int use_min, int* __restrict__ keep,
                                                 int* __restrict__ n_keep) {
    PostLds& L = *(PostLds*)post_smem;
    const int tid = threadIdx.x;
    if (n == 0) { if (tid == 0) *n_keep = 0; return; }
    const int p2 = np2_of(n);
    for (int i = tid; i < p2; i += NT) L.key[i] = i < n ? make_key((float)boxes[(size_t)i * 5 + 4], (unsigned)i) : ~0ull;
    __syncthreads();
    sort_keys(L, p2);
    for (int i = tid; i < n; i += NT) {
        const double* b = boxes + (size_t)key_idx(L.key[i]) * 5;
        L.x1[i] = b[0]; L.y1[i] = b[1]; L.x2[i] = b[2]; L.y2[i] = b[3];
        L.area[i] = __dmul_rn(b[2] - b[0] + 1.0, b[3] - b[1] + 1.0);
    }
    __syncthreads();
    nms_sorted(L, n, thr, use_min != 0);
    for (int k = tid; k < L.nkeep; k += NT) keep[k] = (int)key_idx(L.key[L.keep_pos[k]]);
    if (tid == 0) *n_keep = L.nkeep;
}

template <class K>
int set_lds(K kernel) {      // (every launch: the attribute is per device, the calls are a few per frame)
    HSEFR_HIP_CHECK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PostLds)));
    return HSEFR_OK;
}

}  // namespace

int mtcnn_post_capacity() { return CAP; }

int launch_mtcnn_stage1_level(const float* prob, const float* reg, int w, int h, double scale, float thr, double* found, int* counters,
                              hipStream_t s) {
    return launch_mtcnn_stage1_level_batch(prob, reg, 1, w, h, scale, thr, found, counters, s);
}

int launch_mtcnn_stage1_finish(const double* found, int* counters, double* boxes, int* tab, int img_w, int img_h, hipStream_t s) {
    return launch_mtcnn_stage1_finish_batch(found, counters, boxes, tab, 1, img_w, img_h, s);
}

static int launch_stage23(int stage, const double* boxes_in, int n, const int* offsets, int n_total, const float* prob, const float* reg,
                          const float* pts, float thr, double* boxes_out, int* tab_out, float* points_out, int* counters, int frames, int img_w,
                          int img_h, hipStream_t s) {
    if (stage == 2) {
        if (int rc = set_lds(stage23_finish_kernel<2>)) return rc;
        HSEFR_LAUNCH(stage23_finish_kernel<2>, dim3(frames), dim3(NT), sizeof(PostLds), s, boxes_in, n, offsets, n_total, prob, reg, pts, thr,
                           boxes_out, tab_out, points_out, counters, img_w, img_h);
    } else {
        if (int rc = set_lds(stage23_finish_kernel<3>)) return rc;
        HSEFR_LAUNCH(stage23_finish_kernel<3>, dim3(frames), dim3(NT), sizeof(PostLds), s, boxes_in, n, offsets, n_total, prob, reg, pts, thr,
                           boxes_out, tab_out, points_out, counters, img_w, img_h);
    }
    return launch_status("mtcnn_stage_finish");
}

int launch_mtcnn_stage23_finish(int stage, const double* boxes_in, int n, const float* prob, const float* reg, const float* pts, float thr,
                                double* boxes_out, int* tab_out, float* points_out, int* counters, int img_w, int img_h, hipStream_t s) {
    HSEFR_REQUIRE((stage == 2 || stage == 3) && n >= 0, HSEFR_ERR_INVALID, "mtcnn_stage_finish: stage %d, n %d", stage, n);
    return launch_stage23(stage, boxes_in, n, nullptr, n, prob, reg, pts, thr, boxes_out, tab_out, points_out, counters, 1, img_w, img_h, s);
}

int launch_mtcnn_stage1_level_batch(const float* prob, const float* reg, int frames, int w, int h, double scale, float thr, double* found,
                                    int* counters, hipStream_t s) {
    HSEFR_REQUIRE(frames >= 1 && w > 0 && h > 0 && scale > 0 && (long long)w * h < (1ll << 31), HSEFR_ERR_INVALID,
                  "mtcnn_stage1_level: %d frames, bad map %dx%d", frames, w, h);
    if (int rc = set_lds(stage1_level_kernel)) return rc;
    HSEFR_LAUNCH(stage1_level_kernel, dim3(frames), dim3(NT), sizeof(PostLds), s, prob, reg, w, h, scale, thr, found, counters);
    return launch_status("mtcnn_stage1_level");
}

int launch_mtcnn_stage1_finish_batch(const double* found, int* counters, double* boxes, int* tab, int frames, int img_w, int img_h, hipStream_t s) {
    HSEFR_REQUIRE(frames >= 1, HSEFR_ERR_INVALID, "mtcnn_stage1_finish: %d frames", frames);
    if (int rc = set_lds(stage1_finish_kernel)) return rc;
    HSEFR_LAUNCH(stage1_finish_kernel, dim3(frames), dim3(NT), sizeof(PostLds), s, found, counters, boxes, tab, img_w, img_h);
    return launch_status("mtcnn_stage1_finish");
}

int launch_mtcnn_stage23_finish_batch(int stage, const double* boxes_in, const int* offsets, const float* prob, const float* reg, const float* pts,
                                      float thr, double* boxes_out, int* tab_out, float* points_out, int* counters, int frames, int n_total, int img_w,
                                      int img_h, hipStream_t s) {
    HSEFR_REQUIRE((stage == 2 || stage == 3) && frames >= 1 && n_total >= 0 && offsets, HSEFR_ERR_INVALID,
                  "mtcnn_stage_finish: stage %d, %d frames, %d rows", stage, frames, n_total);
    return launch_stage23(stage, boxes_in, 0, offsets, n_total, prob, reg, pts, thr, boxes_out, tab_out, points_out, counters, frames, img_w, img_h, s);
}

int launch_mtcnn_nms(const double* boxes, int n, double thr, int use_min, int* keep, int* n_keep, hipStream_t s) {
    HSEFR_REQUIRE(n >= 0 && n <= CAP, HSEFR_ERR_UNSUPPORTED, "mtcnn_nms: %d boxes (capacity %d)", n, CAP);
    if (int rc = set_lds(nms_kernel)) return rc;
    HSEFR_LAUNCH(nms_kernel, dim3(1), dim3(NT), sizeof(PostLds), s, boxes, n, thr, use_min, keep, n_keep);
    return launch_status("mtcnn_nms");
}

}  // namespace hsefr
