/*
 * hsefr_affinity.h -- C ABI of libhsefr_affinity.so: affinity-propagation clustering of face features on the device, the last of the three
 * fits the clustering study's scikit-learn branch names (age_gender_identity/facial_clustering_test.py:210, :263:
 * AffinityPropagation().fit(all_features)) and the one method of the study that takes neither a threshold nor a bandwidth
 * (hse_facerec_tf_amd/clustering.py: affinity_propagation, affinity_propagation_dense, affinity_propagation_predict,
 * cluster_faces_affinity_propagation, affinity_propagation_scores).
 *
 * What it replaces in the reference: sklearn.cluster.AffinityPropagation(damping, max_iter, convergence_iter, preference).fit(X) as
 * scikit-learn 1.7.2 executes it (sklearn/cluster/_affinity_propagation.py; tests/affinity_ref.py restates it in NumPy), operation by
 * operation in fp64, on an input of fp64: the fp32 features are widened exactly and the similarities, the preference and the messages
 * are doubles.  scikit-learn itself keeps an fp32 input's similarities in fp32 and perturbs them at fp32's eps; what this library
 * answers is AffinityPropagation(...).fit(X.astype(np.float64)).
 *
 * The tenth library of the package (hse_facerec_tf_amd/_lib.py: LIBRARIES; csrc/build.sh: LIBS): a library of its own as the nine
 * before it -- nothing is shared but the status values of hsefr.h, its own version and per-thread error string.
 *
 * Conventions: those of hsefr.h, whose status values this header uses -- extern "C", plain C types, 0 on success or a negative
 * hsefr_status, never throws, data pointers are DEVICE pointers owned by the caller, `stream` is a hipStream_t.  Built for gfx950 only.
 */
#ifndef HSEFR_AFFINITY_H
#define HSEFR_AFFINITY_H

#include <stddef.h>
#include <stdint.h>

#include "hsefr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSEFR_AFFINITY_VERSION 100

/* limits, refused beyond them with HSEFR_ERR_UNSUPPORTED */
#define HSEFR_AFFINITY_MAX_N 16384       /* points: a row of n doubles lies in a workgroup's LDS (128 KiB of the CU's 160) beside the scratch */
#define HSEFR_AFFINITY_MAX_D 4096        /* d is a multiple of HSEFR_AFFINITY_D_MULTIPLE: 4 .. HSEFR_AFFINITY_MAX_D */
#define HSEFR_AFFINITY_D_MULTIPLE 4
#define HSEFR_AFFINITY_MAX_ITER 10000    /* max_iter: 1 .. HSEFR_AFFINITY_MAX_ITER */
#define HSEFR_AFFINITY_MAX_CONVERGENCE_ITER 64   /* convergence_iter: 1 .. 64, one bit of a 64-bit history word per iteration and point */

/* the words of `info` (8 int32) */
enum {
    HSEFR_AFFINITY_INFO_CLUSTERS = 0,    /* K: the entries of `exemplars` that were written (0: no exemplar, every label is -1) */
    HSEFR_AFFINITY_INFO_N_ITER = 1,      /* scikit-learn's n_iter_: it + 1 of the last iteration run; 0 for equal similarities */
    HSEFR_AFFINITY_INFO_CONVERGED = 2,   /* 1: the stop test held (or the similarities were equal); 0: max_iter iterations ran without it */
    HSEFR_AFFINITY_INFO_EQUAL = 3,       /* 1: n == 1 or all off-diagonal similarities equal: answered without iterating */
    HSEFR_AFFINITY_INFO_NONFINITE = 4,   /* 1: a NaN or an infinity in the input; refused, nothing else was computed */
    HSEFR_AFFINITY_INFO_INTERNAL = 5,    /* 1: an index left its bound on the device; it was not followed, and the call failed */
    HSEFR_AFFINITY_INFO_WORDS = 8
};

/*
 * The noise.  scikit-learn adds (eps S + 100 tiny) N(0, 1) from a generator that is unseeded by default, so that exact ties (duplicated
 * rows; the two members of a two-point cluster) fall one way or the other.  Here the factor is a counter hash of (seed, the entry's
 * flat index e = i n + j), of unit variance, uniform on (-sqrt 3, sqrt 3):
 *
 *     z = (uint64) e + (uint64) seed * HSEFR_AFFINITY_HASH_SEED_MUL + HSEFR_AFFINITY_HASH_GAMMA       (mod 2^64)
 *     z = (z ^ (z >> 30)) * HSEFR_AFFINITY_HASH_MUL1;  z = (z ^ (z >> 27)) * HSEFR_AFFINITY_HASH_MUL2;  z = z ^ (z >> 31)      (splitmix64)
 *     g = (((double)(z >> 12) + 0.5) * 2^-52 * 2.0 - 1.0) * HSEFR_AFFINITY_SQRT3
 *     S[e] = S[e] + (2^-52 * S[e] + 100.0 * DBL_MIN) * g
 *
 * every operation rounded on its own (no fused multiply-add), so that NumPy gives the same bits (tests/affinity_ref.py: noise_factor).
 * The noise is added to the whole matrix after the preference stands on the diagonal, as scikit-learn does; noise_seed = -1 adds nothing.
 */
#define HSEFR_AFFINITY_HASH_SEED_MUL 0xD1342543DE82EF95ull
#define HSEFR_AFFINITY_HASH_GAMMA 0x9E3779B97F4A7C15ull
#define HSEFR_AFFINITY_HASH_MUL1 0xBF58476D1CE4E5B9ull
#define HSEFR_AFFINITY_HASH_MUL2 0x94D049BB133111EBull
#define HSEFR_AFFINITY_SQRT3 1.7320508075688772

/*
 * The arithmetic.  On the features path S_ij = 0 - max(0, fl(N_i + N_j) - 2 P_ij) and S_ii = 0, with P the fp64 MFMA product
 * (v_mfma_f64_16x16x4_f64: d multiply-adds into one accumulator, the same products in the same order for P_ij and P_ji: S is symmetric bit
 * for bit) and N_i = sum x_ik^2 over 64 interleaved partial sums.  As in hsefr_shift.h, with u = 2^-53,
 *
 *     | S_ij + |x_i - x_j|^2 |   <=   HSEFR_AFFINITY_SIM_ULPS(d) * 2^-53 * (|x_i| + |x_j|)^2 .
 *
 * The default preference is np.median of all n^2 entries, EXACT: a radix select on order-preserving 64-bit keys finds the two middle
 * entries (the same entry twice for an odd count) and the preference is their fp64 mean.  Every update of an iteration is scikit-learn's
 * expression with scikit-learn's roundings; the one difference from NumPy is the ORDER of the column sums of max(R, 0): a workgroup adds
 * its block of rows in index order and the blocks' partial sums are added in one fixed order (four running sums over the blocks, then
 * their sum; no floating-point atomics: two runs give identical bytes).  On an input where every operation is exact (small integers, damping 0.5) the result is NumPy's bit for bit.
 *
 * How far a message can lie from scikit-learn's, to first order.  While the two computations select the same entries (each row's
 * argmax, the signs of R, the clipped entries of A -- what the margins of tests/affinity_ref.py guard), a message of any iteration is a
 * signed sum of similarities and of earlier messages: a responsibility of two entries of A + S, an availability of at most n clipped
 * responsibilities, and the damping makes every generation a convex combination of the one before and that sum.  An error of
 * HSEFR_AFFINITY_SIM_ULPS(d) u in every similarity, n u of a column sum's value from the order of its n additions and the 16 u of the
 * updates' own roundings therefore move A_kk + R_kk, a member sum of the refinement or the similarity a point is assigned by, by at most
 *
 *     HSEFR_AFFINITY_MSG_ULPS(n, d) * 2^-53 * max |S|          (max over the entries, the preference among them)
 *
 * (ops.affinity_message_bound states it in Python: 8e-11 at n = 1926, d = 64, max |S| = 4).  It is a first-order bound, not a proof
 * over all inputs: the recorder of the test cases (tools/record_affinity_golden.py) keeps a case only if scikit-learn's partition, n_iter_
 * and cluster count also survive a relative perturbation of S by 1e-11, 10^4 times the similarities' error, and the GPU tests compare
 * with scikit-learn only after asserting that the least |A_kk + R_kk| of all iterations and the least assignment gap are 100 times this bound.
 */
#define HSEFR_AFFINITY_SIM_ULPS(d) ((d) + 8)
#define HSEFR_AFFINITY_MSG_ULPS(n, d) ((n) * ((d) + 24))

int hsefr_affinity_version(void);

/* the last failure on the calling thread ("" before the first) */
const char* hsefr_affinity_last_error(void);

/* bytes of workspace a fit needs for n points of d features (three n x n fp64 matrices, the row blocks' partial column sums and O(n)
 * words; hsefr_affinity_fit_dense: the same with any supported d); 0 for an n or d that is refused */
size_t hsefr_affinity_workspace_bytes(int n, int d);

/*
 * AffinityPropagation(damping, max_iter, convergence_iter, preference).fit(x.astype(float64)): x [n, d] fp32, never written.
 *   damping           0.5 <= damping < 1
 *   preference_in     the preference, one double; a NaN: np.median of the similarities (scikit-learn's preference=None)
 *   noise_seed        >= 0: the seed of the noise above; -1: no noise
 *   exemplars         int32 [n]: the first info[0] entries are cluster_centers_indices_, ascending; the others are not written
 *   labels            int32 [n]: the position in `exemplars` of the point's exemplar; all -1 when info[0] is 0
 *   diag              fp64 [n]: A_kk + R_kk after the last iteration (its sign is the exemplar decision); zeros for equal similarities
 *   preference        fp64 [1]: the preference that stood on the diagonal
 *   info              int32 [8]: HSEFR_AFFINITY_INFO_*
 *   workspace         at least hsefr_affinity_workspace_bytes(n, d) bytes, 16-byte aligned (x: 8-byte aligned)
 * An iteration is three launches (the row sweeps, the column sums with the history and the stop test); the call synchronises `stream`
 * once per iteration (it reads 64 bytes: whether to stop) and returns with it drained.  Every loop on the host and the device is bounded
 * by max_iter or n.  A loop that runs max_iter iterations without the stop test holding is "not converged" (scikit-learn's ConvergenceWarning).
 *
 * HSEFR_ERR_INVALID before any device work, with a message that starts with "affinity_": a null pointer, n < 1, damping outside
 * [0.5, 1), convergence_iter outside 1 .. 64, an infinite preference_in, noise_seed < -1, a workspace that is too small or misaligned.
 * HSEFR_ERR_UNSUPPORTED before any device work: n, d or max_iter beyond the limits above.
 * HSEFR_ERR_INVALID with info[4] = 1 for a non-finite input; HSEFR_ERR_HIP with info[5] = 1 should an index leave its bound.
 */
int hsefr_affinity_fit(const float* x, int n, int d, double damping, int max_iter, int convergence_iter, double preference_in,
                       long long noise_seed, int32_t* exemplars, int32_t* labels, double* diag, double* preference, int32_t* info,
                       void* workspace, size_t workspace_bytes, void* stream);

/*
 * affinity="precomputed": the same over a caller's similarities s [n, n] fp64, which may be asymmetric and are never written (they are
 * copied into the workspace: hsefr_affinity_workspace_bytes(n, HSEFR_AFFINITY_D_MULTIPLE) bytes).  Everything else as above.
 */
int hsefr_affinity_fit_dense(const double* s, int n, double damping, int max_iter, int convergence_iter, double preference_in,
                             long long noise_seed, int32_t* exemplars, int32_t* labels, double* diag, double* preference, int32_t* info,
                             void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif
