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

#ifdef HSEFR_GEOM_LIB
// libhsefr_geom.so (include/hsefr_geom.h) compiles hier_linkage.hip a second time under this macro and takes from it, besides the build:
//   rescan_rows          hl_rescan_kernel on `blocks` workgroups: nn / nnd of the rows list[0 .. cnt[HL_CNT_LIST]) over the alive columns,
//                        least (value, column); a no-op while cnt[HL_CNT_ALIVE] <= 1.  cnt: a block of HL_CNT_WORDS ints of the caller's;
//   launch_ward_linkage  launch_hier_linkage with Ward's rule; w_out (optional) receives W as first built, counts (optional, device)
//                        {records written, radicands clamped at zero}.
constexpr int HL_CNT_ALIVE = 0, HL_CNT_LIST = 4, HL_CNT_WORDS = 8;
void rescan_rows(const double* W, int n, const int* alive, const int* list, const int* cnt, int* nn, double* nnd, int blocks, hipStream_t s);
int launch_ward_linkage(const DistSource& src, int* merge_a, int* merge_b, double* merge_h, int* merge_round, double* w_out, long long* counts,
                        hipStream_t s);
#endif

}  // namespace hsefr
