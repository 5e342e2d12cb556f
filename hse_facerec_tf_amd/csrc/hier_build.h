// The fp64 n x n working matrix shared by hier_linkage.hip (average / complete / weighted linkage) and rank_order.hip, from one of two
// sources:
//   features  W[i,j] = w(i,j) of linkage_scan.h (feat_tile: the one feature tile the row scans of single linkage and DBSCAN use too)
//             widened to fp64; each 32 x 32 tile of the upper triangle is computed once and stored to both sides through LDS;
//   dense     a caller's fp64 D [n,n], read as its upper triangle D[min(i,j), max(i,j)] (what squareform(D, checks=False) reads),
//             copied to both sides; the caller's buffer is never written.
// W is bitwise symmetric and its diagonal +inf.  The kernels live in hier_linkage.hip; nothing is synchronised.
#pragma once
#include "common.h"

namespace hsefr {

// Launches the build of W (n^2 doubles) from src on s; the caller's launch_status covers it.
void build_working_matrix(const DistSource& src, double* W, hipStream_t s);

}  // namespace hsefr
