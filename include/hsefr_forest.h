/*
 * hsefr_forest.h -- C ABI of libhsefr_forest.so: a random forest classifier fitted and applied on the device, the 'rf' row of the
 * reference's classifier table (facerec_test.py:269-282, RandomForestClassifier(n_estimators=100, max_depth=10)).
 *
 * scikit-learn's forest is not a function of its inputs (no random_state in the reference, and a sequential generator consumed in
 * depth-first build order), so this forest has a definition of its own: a pure function of (x, labels, n_trees, max_depth,
 * max_features, bootstrap, seed), restated in NumPy in tests/random_forest_ref.py, which the device equals bit for bit.
 *
 * The definition, once (the restatement words it the same way):
 *   hash       mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31 (splitmix64's
 *              finaliser).  hash(seed, tree, purpose, node, counter): h = mix(seed + G); then for v in (tree, purpose, node, counter):
 *              h = mix(h + v + G); G = 0x9E3779B97F4A7C15; uint64 with wrap-around.  purpose 1 = bootstrap, 2 = feature order.
 *   bootstrap  row j of tree t is ((hash(seed, t, 1, 0, j) >> 32) * n) >> 32; a row's multiplicity is its integer weight; rows with
 *              multiplicity 0 are not in the tree; bootstrap == 0 gives every row weight 1.
 *   nodes      numbered as a heap for the hash (root 1, children 2 i and 2 i + 1) and STORED level by level: node 0 is the root, the
 *              children of a level's split nodes follow in that level's order, left before right.  A tree's distinct rows stay
 *              partitioned: a node holds a contiguous segment (ascending row index at the root); a split moves the rows with
 *              (double) x <= threshold to the segment's front, both halves keeping their order.
 *   features   of a node are visited by ascending ((hash(seed, tree, 2, node, f) >> 12 << 12) | f) -- the hash's upper 52 bits, then
 *              f.  The first max_features are all visited; while no candidate has been seen the visit goes on feature by feature
 *              until one yields a candidate or all d are exhausted.
 *   split      the node's rows sorted by the feature's value; position p (1 <= p < rows) is a candidate iff v[p] > v[p-1] (what
 *              the installed scikit-learn 1.7.2 build's splitter does: its FEATURE_THRESHOLD, 1e-7 in the source, is 0 where it is
 *              used, measured by tools/record_random_forest_golden.py; a later scikit-learn that restores the 1e-7 would show as that
 *              recorder no longer reproducing tests/golden/random_forest.npz).  Score:
 *              S_L / N_L + S_R / N_R in fp64, S the sum of squared weighted class counts and N the weighted count of a side, both
 *              integers.  The largest wins; equal scores go to the earlier feature of the visit, then the lower position.
 *              threshold = (double) v[p-1] / 2.0 + (double) v[p] / 2.0, or v[p-1] where that equals v[p] or is not finite.
 *   leaves     at max_depth, with fewer than 2 distinct rows, with one class only, or without a candidate.  A leaf keeps (class,
 *              weighted count) pairs by ascending class at [leaf_begin, leaf_begin + leaf_len) of its tree's list; leaf_begin is the
 *              start of its segment.
 *   predict    proba[c] = (sum over trees of count_t[c] / N_t) / n_trees in fp64, the terms added in tree order from 0.0; the label
 *              is the largest, equal values to the lowest class.
 *
 * A fourth library, as libhsefr_album.so and libhsefr_frames.so are: libhsefr.so stays as it is (its size is bounded by its tests)
 * and the four share no symbol -- this one has its own version number and its own per-thread error string.
 *
 * Conventions: those of hsefr.h -- extern "C", plain C types, 0 on success or a negative status (the values of hsefr_status), never
 * throws, data pointers are DEVICE pointers owned by the caller, launches are asynchronous on `stream` (a hipStream_t passed as
 * void*; NULL = the default stream), nothing is allocated and nothing synchronises.  Built for gfx950 only.
 */
#ifndef HSEFR_FOREST_H
#define HSEFR_FOREST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSEFR_FOREST_VERSION 100

#define HSEFR_FOREST_OK 0
#define HSEFR_FOREST_ERR_INVALID (-1)     /* bad argument                              */
#define HSEFR_FOREST_ERR_UNSUPPORTED (-2) /* a size over the limits below              */
#define HSEFR_FOREST_ERR_HIP (-3)         /* a HIP runtime call failed                 */

/* the limits of fit and predict (LFW's gallery half -- n = 4582, d = 1024, 1680 classes, 100 trees, depth 10 -- lies inside) */
#define HSEFR_FOREST_MAX_N 65535        /* rows: a side's sum of squared counts stays below 2^32 */
#define HSEFR_FOREST_MAX_D 4096         /* features: the visiting key keeps 12 bits for f        */
#define HSEFR_FOREST_MAX_CLASSES 2048   /* a node's class counts live in LDS                     */
#define HSEFR_FOREST_MAX_TREES 1024
#define HSEFR_FOREST_MAX_DEPTH 24
#define HSEFR_FOREST_MAX_CANDIDATES (1ll << 28) /* n_trees * min(2^(max_depth-1), n) * max_features, the candidate table's rows */
#define HSEFR_FOREST_MAX_SLAB_BYTES (1ll << 32) /* n > 4096 only: n_trees * max_features * 2 n * 8, the global-memory sort's space */
#define HSEFR_FOREST_MAX_PROBES (1 << 24)

/* bits of d_info[0] after a fit */
#define HSEFR_FOREST_INFO_BAD_LABEL 1   /* a label outside 0..n_classes-1                                      */
#define HSEFR_FOREST_INFO_NOT_FINITE 2  /* a NaN or an infinity in x                                           */
#define HSEFR_FOREST_INFO_INTERNAL 4    /* an index derived from data left its bound (not written; a bug)      */

int hsefr_forest_version(void);

/* the last failure on the calling thread ("" before the first) */
const char* hsefr_forest_last_error_string(void);

/*
 * Bytes of d_workspace that hsefr_forest_fit needs for these sizes; 0 where fit would refuse them (the error string says why).
 * Rows larger than 4096 (one sort tile in LDS) add n_trees * max_features * 2 n 8-byte keys for the sort in global memory.
 */
size_t hsefr_forest_workspace_bytes(int n, int d, int n_trees, int max_depth, int max_features);

/*
 * Fits the forest defined above.
 *   d_x        DEVICE float32 [n, d], finite          d_labels  DEVICE int32 [n], codes in 0..n_classes-1 (a class may have no row)
 *   max_features in 1..d; bootstrap 0 or 1; seed below 2^63
 *   node_capacity  must be min(2^(max_depth+1) - 1, 2 n - 1): the worst case of a tree, the stride of the node arrays
 * Outputs, all DEVICE, a tree's slice at [tree * node_capacity] (nodes) or [tree * n] (leaf lists); slots past a tree's node count
 * hold -1 (thresholds 0.0), unused leaf entries class -1 and count 0:
 *   d_feature int32 (-1: a leaf), d_threshold float64, d_left / d_right int32 (node indices inside the tree, -1 at a leaf),
 *   d_weight int32 (the node's weighted row count N), d_leaf_begin / d_leaf_len int32 (leaves only), d_leaf_class / d_leaf_count
 *   int32 [n_trees, n], d_n_nodes int32 [n_trees], d_info int32 [4] ([0]: the HSEFR_FOREST_INFO_ bits, 0 after a good fit; the
 *   caller reads it back: with a bit set the forest is not to be used).
 * Every argument is checked before any device work: HSEFR_FOREST_ERR_INVALID for a null pointer, a size below 1 (n_classes below 2),
 * max_features outside 1..d, a negative seed, a wrong node_capacity or a workspace smaller than hsefr_forest_workspace_bytes();
 * HSEFR_FOREST_ERR_UNSUPPORTED beyond the limits above.  Integer counts and fp64 scores, no floating-point atomics: two fits
 * give identical bytes.
 */
int hsefr_forest_fit(const float* d_x, int n, int d, const int32_t* d_labels, int n_classes, int n_trees, int max_depth, int max_features,
                     int bootstrap, long long seed, int node_capacity, int32_t* d_feature, double* d_threshold, int32_t* d_left,
                     int32_t* d_right, int32_t* d_weight, int32_t* d_leaf_begin, int32_t* d_leaf_len, int32_t* d_leaf_class,
                     int32_t* d_leaf_count, int32_t* d_n_nodes, int32_t* d_info, void* d_workspace, size_t workspace_bytes, void* stream);

/*
 * Applies a forest to the probes d_q (DEVICE float32 [nq, d]): d_labels int32 [nq] always, d_proba float64 [nq, n_classes] unless
 * NULL.  The node arrays are plain device buffers in the layout of hsefr_forest_fit with strides node_capacity (nodes) and
 * leaf_capacity (leaf lists), so a forest from elsewhere can be run; every index read from them is checked against its bound
 * before it is used, and a probe that meets a bad one (a child or feature out of range, a walk longer than node_capacity, a leaf
 * list past leaf_capacity, a weight below 1) is labelled -1.  One workgroup per probe with the probabilities in LDS.
 * HSEFR_FOREST_ERR_INVALID / _UNSUPPORTED as for fit (nq in 1..HSEFR_FOREST_MAX_PROBES, node_capacity and leaf_capacity at least 1).
 */
int hsefr_forest_predict(const float* d_q, int nq, int d, int n_classes, int n_trees, int node_capacity, int leaf_capacity,
                         const int32_t* d_feature, const double* d_threshold, const int32_t* d_left, const int32_t* d_right,
                         const int32_t* d_weight, const int32_t* d_leaf_begin, const int32_t* d_leaf_len, const int32_t* d_leaf_class,
                         const int32_t* d_leaf_count, double* d_proba, int32_t* d_labels, void* stream);

#ifdef __cplusplus
}
#endif

#endif
