// The three geometric Lance-Williams rules of libhsefr_geom.so (include/hsefr_geom.h), stated once for the rounds of hier_linkage.hip
// (Ward) and the closest-pair engine of geom_linkage.hip (centroid, median).
//
// They are scipy's _hierarchy_distance_update.pxi operation by operation, in fp64 and without contraction, so the roundings are scipy's:
// x and y are the clusters that merge, i the third one, d.. their distances, s. their sizes.  The one thing of ours is the clamp: a
// radicand that rounding, or a matrix that is not Euclidean (the age term), makes negative gives 0 where scipy's sqrt gives NaN, and
// every such radicand counts one in `clamps`.  Wherever scipy's value is a number this is that number.
#pragma once
#include <hip/hip_runtime.h>

namespace hsefr {
namespace geom {

__device__ __forceinline__ double clamped_root(double r, unsigned& clamps) {
    if (r < 0.0) ++clamps;
    return sqrt(fmax(r, 0.0));
}

__device__ __forceinline__ double centroid(double dxi, double dyi, double dxy, int sx, int sy, unsigned& clamps) {
#pragma clang fp contract(off)
    const double fx = (double)sx, fy = (double)sy, fxy = (double)((long long)sx * sy), fs = (double)(sx + sy);
    const double r = ((fx * dxi * dxi + fy * dyi * dyi) - (fxy * dxy * dxy) / fs) / fs;
    return clamped_root(r, clamps);
}

__device__ __forceinline__ double median(double dxi, double dyi, double dxy, unsigned& clamps) {
#pragma clang fp contract(off)
    const double r = 0.5 * (dxi * dxi + dyi * dyi) - 0.25 * dxy * dxy;
    return clamped_root(r, clamps);
}

__device__ __forceinline__ double ward(double dxi, double dyi, double dxy, int sx, int sy, int si, unsigned& clamps) {
#pragma clang fp contract(off)
    const double t = 1.0 / (double)(sx + sy + si);
    const double r = (double)(si + sx) * t * dxi * dxi + (double)(si + sy) * t * dyi * dyi - (double)si * t * dxy * dxy;
    return clamped_root(r, clamps);
}

}  // namespace geom
}  // namespace hsefr
