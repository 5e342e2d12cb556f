// The fp32 MFMA contraction of a 32 x 32 tile shared by nn1.hip (nn1_kernel, pairwise_dist_kernel) and the clustering feature tile of
// linkage_scan.h.  One wave = 32 rows of A against 32 rows of B over d (a multiple of 8): lane (li, lh) streams row li of each operand
// from element 4 lh on (ap / bp point there), 4 of every 8 elements, and ends with acc[r] = a_row(r) . b_li for the 16 tile rows
// row(r) = (r & 3) + 8 (r >> 2) + 4 lh, and with its half of |a_li|^2 and |b_li|^2, summed from the very fragments that feed the MFMAs
// (the other half is lane li of the other half-wave: __shfl_xor(., 32)).  A wave with on == false (wave-uniform) contracts nothing and
// ends with zeros.  Each caller keeps its own epilogue.
#pragma once
#include <hip/hip_runtime.h>

namespace hsefr {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ void mfma_dot_32x32(const float* ap, const float* bp, int d, f32x16& acc, float& aa, float& bb, bool on = true) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    aa = 0.f;
    bb = 0.f;
    for (int k = 0; on && k < d; k += 8) {
        const f32x4 a = *(const f32x4*)(ap + k);
        const f32x4 b = *(const f32x4*)(bp + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
            bb = fmaf(b[j], b[j], bb);
            aa = fmaf(a[j], a[j], aa);
        }
    }
}

}  // namespace hsefr
