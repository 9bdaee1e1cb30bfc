/*
 * gkm_svm.h -- GPU-resident consumer of the gkm kernel matrix: C-SVC
 * training and decision values on a PRECOMPUTED kernel that already sits in HBM, for the
 * cross-validation gkmQC runs on every matrix (reference scripts/gkmsvm.py:104-176:
 * StratifiedKFold x repeats -> sklearn.svm.SVC(kernel="precomputed") -> decision_function).
 *
 * What it replaces: the LIBSVM solver inside scikit-learn (sklearn/svm/src/libsvm/svm.cpp,
 * `Solver::Solve` with second-order working-set selection; gkmsvm_train_batch without the shrinking
 * heuristic -- gkmQC's default `--shrinking 0` --, gkmsvm_train_batch_general with or without it).  That code is a third-party dependency of the reference, not part of
 * /root/reference; the algorithm restated here is Fan, Chen, Lin (2005) "Working set selection
 * using second order information" as implemented by LIBSVM 3.x: same iteration sequence, same
 * tie breaking, kernel values rounded to float as LIBSVM's Qfloat, all other arithmetic fp64.
 * Parity is pinned against scikit-learn itself (tests/test_svm_gpu.py): dual coefficients and
 * intercept bit-identical, AUC identical.
 *
 * All folds of a cross-validation are solved concurrently, one workgroup per fold.
 * Plain pointers and sizes; `K` and every array below are DEVICE pointers unless noted.
 */
#ifndef GKM_SVM_H
#define GKM_SVM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Train nprob independent C-SVC problems on sub-matrices of one symmetric kernel matrix.
 *   K, ld, n     n x n fp64, row-major with leading dimension ld, BOTH triangles filled, device
 *   idx          concatenated training indices (into K) of all problems, each problem in LIBSVM's
 *                internal order: all samples of class 0 first (they get y = +1), then class 1 (y = -1)
 *   off[nprob+1] HOST array: offsets of the problems into idx / alpha / grad
 *   n0[nprob]    HOST array: number of class-0 samples of each problem
 *   C, eps       box constraint and stopping tolerance (sklearn `C`, `tol`)
 *   alpha, grad  out, device, same layout as idx: dual variables (0..C) and final gradient
 *   rho          out, device, nprob doubles
 *   iters        out, device, nprob ints; NEGATIVE when the fold stopped at the iteration cap (10^7, LIBSVM's
 *                classic default; scikit-learn has none): that fold has not converged and must be re-solved
 *                by the caller if the reference's result is wanted
 * Returns 0 on success (work enqueued on `stream`); GKMSVM_RC_SHAPE_REFUSED when the device refuses the launch shape
 * the largest fold needs (its dynamic LDS) -- the one failure after which gkmsvm_train_batch_general is worth trying:
 * it needs no state in LDS (it keeps some there when the device grants it) and returns the same bits without
 * shrinking; any other value is an error of the arguments or of the device.
 */
#define GKMSVM_RC_SHAPE_REFUSED 5
int gkmsvm_train_batch(int device, const double *K, int64_t ld, int n, int nprob, const int *idx, const int64_t *off,
                       const int *n0, double C, double eps, double *alpha, double *grad, double *rho, int *iters,
                       void *stream);

/*
 * The same with LIBSVM's shrinking heuristic (`shrinking` != 0; scikit-learn `SVC(shrinking=True)`, what the
 * reference's `--shrinking 1` selects, scripts/gkmsvm.py:110-118) and for folds of up to 60 000 samples:
 * Solver::Solve restated with do_shrinking / swap_index / reconstruct_gradient / G_bar, one workgroup per fold,
 * state in global memory -- for folds of at most 8 192 samples the part of it every iteration scans (gradient, Q_i,
 * matrix index, one state byte per sample) in LDS instead, 147 KB, if the device grants that.  Bit-identical to
 * scikit-learn with either setting (tests/test_svm_gpu.py); 1.4x (8 000-sample folds) to 2x slower per iteration than
 * gkmsvm_train_batch, which stays the path for gkmQC's default.
 * Environment, for measurements: GKM_SVM_GEN_LDS=0 (state in global memory always), GKM_SVM_GEN_T=512|1024 (threads).
 */
int gkmsvm_train_batch_general(int device, const double *K, int64_t ld, int n, int nprob, const int *idx,
                               const int64_t *off, const int *n0, double C, double eps, int shrinking, double *alpha,
                               double *grad, double *rho, int *iters, void *stream);

/*
 * The two entries above with a box per problem and per class instead of one C per launch (LIBSVM's `-wi`, scikit-learn's
 * `class_weight`, and a grid of C values in one launch):
 *   box          HOST array, nprob x 2 doubles: box[2p] bounds the class-0 positions of problem p (the first n0[p], y = +1),
 *                box[2p + 1] the rest -- LIBSVM's Cp = C * weight[0] and Cn = C * weight[1] in this order of the classes.
 *                alpha of a position lies in 0..its class's bound.
 * Everything else -- arguments, size limits (16 384 / 60 000 samples), outputs, iteration cap, GKMSVM_RC_SHAPE_REFUSED,
 * the scratch pool, the environment knobs -- is as for the unboxed entries, and with box[2p] == box[2p + 1] == C the
 * results are their bits.  A bound that is not finite or not > 0 returns 2 and writes nothing.  The unboxed entries run
 * kernel instantiations of their own, which never read a box.
 */
int gkmsvm_train_batch_boxed(int device, const double *K, int64_t ld, int n, int nprob, const int *idx, const int64_t *off,
                             const int *n0, const double *box, double eps, double *alpha, double *grad, double *rho,
                             int *iters, void *stream);
int gkmsvm_train_batch_general_boxed(int device, const double *K, int64_t ld, int n, int nprob, const int *idx,
                                     const int64_t *off, const int *n0, const double *box, double eps, int shrinking,
                                     double *alpha, double *grad, double *rho, int *iters, void *stream);

/*
 * Decision values of problem p for its test samples, in LIBSVM's summation order:
 *   dec[t] = sum_{k in training order, alpha_k > 0} alpha_k y_k K(test_t, train_k) - rho
 * (scikit-learn's decision_function returns the negative of this for a two-class problem).
 *   test_idx / test_off: concatenated test indices per problem (test_off on the HOST).
 */
int gkmsvm_decision_batch(int device, const double *K, int64_t ld, int nprob, const int *idx, const int64_t *off,
                          const int *n0, const double *alpha, const double *rho, const int *test_idx,
                          const int64_t *test_off, double *dec, void *stream);

/*
 * epsilon-SVR (LIBSVM solve_epsilon_svr; scikit-learn SVR(kernel="precomputed")) on the same solvers: each problem of l
 * samples is solved as LIBSVM's 2l-variable problem -- position k < l is sample k with y = +1 and linear term
 * p_k = epsilon - z_k, position l + k the same sample with y = -1 and p_{l+k} = epsilon + z_k (p in fp64 exactly so), alpha
 * starting at 0, box C everywhere.  The entries build that problem themselves (device scratch from the pool).
 *   idx          concatenated training indices (into K) of all problems, each in the caller's order (no reordering)
 *   off[nprob+1] HOST array: offsets of the problems into idx / z / coef
 *   z            device, same layout as idx: the targets
 *   C, epsilon, tol   box constraint, tube half-width, stopping tolerance (scikit-learn `C`, `epsilon`, `tol`)
 *   coef         out, device, same layout as idx: alpha_k - alpha_{l+k} (scikit-learn's dual_coef_ where nonzero)
 *   rho          out, device, nprob doubles: LIBSVM's rho (scikit-learn's intercept_ is -rho)
 *   iters        out, device: as for gkmsvm_train_batch (negative at the iteration cap)
 * gkmsvm_train_svr_batch runs k_smo (2l <= 16 384, no shrinking; GKMSVM_RC_SHAPE_REFUSED as gkmsvm_train_batch),
 * gkmsvm_train_svr_batch_general runs k_smo_general (2l <= 60 000, with or without shrinking).  The environment knobs of
 * the C-SVC entries apply.
 */
int gkmsvm_train_svr_batch(int device, const double *K, int64_t ld, int n, int nprob, const int *idx, const int64_t *off,
                           const double *z, double C, double epsilon, double tol, double *coef, double *rho, int *iters,
                           void *stream);
int gkmsvm_train_svr_batch_general(int device, const double *K, int64_t ld, int n, int nprob, const int *idx,
                                   const int64_t *off, const double *z, double C, double epsilon, double tol,
                                   int shrinking, double *coef, double *rho, int *iters, void *stream);

/*
 * The signed decision of an SVR: dec[t] = sum_{k in order, coef_k != 0} coef_k K(test_t, sv_k) - rho, the additions
 * sequential from +0.0 (scikit-learn's SVR.predict, bit for bit, with rho = -intercept_).  Arguments as for
 * gkmsvm_decision_batch, with the signed coefficients in place of alpha and no n0.
 */
int gkmsvm_decision_signed_batch(int device, const double *K, int64_t ld, int nprob, const int *idx, const int64_t *off,
                                 const double *coef, const double *rho, const int *test_idx, const int64_t *test_off,
                                 double *dec, void *stream);

const char *gkmsvm_last_error(void);

/* The calls above keep their device scratch (problem descriptors, the matrix diagonal, the general solver's state) in a
 * per-process pool instead of allocating and freeing it per call: hipMalloc / hipFree wait for the whole device, i.e. for
 * the Gram kernel of the next subset that a pipeline runs beside the solver (gkmqc_amd/gkmsvm.py init_many).  This frees
 * what is not in use (optional). */
void gkmsvm_release_cache(void);

#ifdef __cplusplus
}
#endif
#endif
