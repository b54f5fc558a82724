/*
 * asvd_hip.h — C ABI of libasvd_hip.so: the MI355X (gfx950) kernels behind the activation-aware SVD
 * compression path of ASVD4LLM.
 *
 * The reference (hahnyuan/ASVD4LLM) is pure Python and has no FFI layer; its arithmetic for this path
 * lives in eager torch ops.  Every entry point below replaces one group of those torch ops; the
 * reference lines are cited per function (paths relative to the reference tree).  A maintainer of the
 * reference binds these with ctypes from inside the same Python functions.
 *
 * Conventions
 *   - plain pointers + sizes; no torch types.  All data pointers are DEVICE pointers unless the name
 *     ends in `_host`.  The caller owns every buffer; the library never frees or retains them.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Kernels are enqueued on it.
 *     Functions documented "host-synchronous" call hipStreamSynchronize(stream) internally because
 *     they return host scalars (sweep counts / NaN flags) or steer iteration on device results.
 *   - return value: 0 = OK; negative = bad argument / runtime error (ASVD_E_*); positive = numerical
 *     condition (ASVD_N_*).  asvd_status_string() gives text.
 *   - matrices are row-major; `ld*` are leading dimensions in ELEMENTS.
 */
#ifndef ASVD_HIP_H
#define ASVD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* element types */
#define ASVD_F32 0
#define ASVD_F16 1
#define ASVD_BF16 2

/* status codes */
#define ASVD_OK 0
#define ASVD_E_BADARG (-1)
#define ASVD_E_WORKSPACE (-2)   /* workspace too small */
#define ASVD_E_HIP (-3)         /* a HIP runtime call failed */
#define ASVD_E_NODEVICE (-4)    /* no gfx950 device visible */
#define ASVD_N_NOCONV 1         /* Jacobi did not reach tol within max_sweeps (results still usable) */
#define ASVD_N_NAN 2            /* NaN/Inf seen in outputs */

/* sigma_fuse modes of SVDLinear.__init__ (modules/svd_linear.py:16-24) */
#define ASVD_FUSE_UV 0
#define ASVD_FUSE_U 1
#define ASVD_FUSE_V 2

/* activation-statistic modes of the calibration hook (act_aware_utils.py:64-74) */
#define ASVD_STAT_ABS_MEAN 0
#define ASVD_STAT_ABS_MAX 1
/* column mean of x^2 with x^2 rounded to the dtype of x first: `weight.grad.pow(2).mean(0)` of calib_fisher_info (act_aware_utils.py:30) */
#define ASVD_STAT_SQ_MEAN 2

int asvd_version(void);
const char* asvd_status_string(int status);
/* number of visible HIP devices with arch gfx950; <=0 means the library cannot run */
int asvd_device_count(void);

/* ---------------------------------------------------------------------------------------------
 * K1/K2  calibration hook accumulator.
 * Replaces act_aware_utils.py:66-67 (abs_mean: `input[0].abs().mean(dim=-2).view(-1)`; `acc += ...`)
 * and :69-74 (abs_max: `.abs().amax(dim=-2)`; `torch.where(abs_max > acc, abs_max, acc)`).
 *   x   [rows, cols] row-major with leading dimension ld (the [1,T,C] / [T,C] hook input flattened)
 *   acc [cols] in acc_dtype (the reference keeps the activation dtype); caller zero-initialises it,
 *       which reproduces the reference's python-int 0 start exactly (0 + x == x; max(x,0) == x).
 * abs_mean: column sums accumulate in fp32, are divided by rows, rounded to acc_dtype, then added to
 *           acc in acc_dtype arithmetic (one rounding), i.e. the reference's two-op sequence.
 * abs_max : NaN in x never replaces acc (torch.where(nan > acc) is false).
 * sq_mean : as abs_mean with x*x (rounded to x's dtype, as torch's .pow(2) does) in place of |x|; x = weight.grad [out, in].
 * work: asvd_absstat_worksize bytes (fp32 partial sums). Asynchronous on `stream`.
 */
int asvd_absstat_worksize(int64_t rows, int64_t cols, size_t* bytes);
int asvd_absstat_accum(const void* x, int x_dtype, int64_t rows, int64_t cols, int64_t ld,
                       void* acc, int acc_dtype, int mode, void* work, size_t work_bytes, void* stream);
/* The two halves of asvd_absstat_accum, for Linears that are called with the SAME input tensor (q/k/v_proj, gate/up_proj: the
 * reference's hook re-reads X for each of them, act_aware_utils.py:78-81): asvd_absstat_partial makes the one pass over X
 * (fp32 partial column statistics into `work`), asvd_absstat_finalize applies them to one accumulator with the arithmetic
 * described above — call it once per Linear sharing the input.  Both asynchronous on `stream`. */
int asvd_absstat_partial(const void* x, int x_dtype, int64_t rows, int64_t cols, int64_t ld, int mode,
                         void* work, size_t work_bytes, void* stream);
int asvd_absstat_finalize(const void* work, size_t work_bytes, int64_t rows, int64_t cols,
                          void* acc, int acc_dtype, int mode, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K3a  scale vector.  Replaces svd_linear.py:48-59:
 *   s = 1 * scaling_diag_matrix**alpha [* fisher_info**alpha]; s += 1e-6
 * evaluated in the dtype of the statistics (fp16 for an fp16 model: pow, product and +eps each round
 * to that dtype, as torch does).  fisher may be NULL.  out has the same dtype.  Asynchronous.
 */
int asvd_make_scale(const void* scaling, const void* fisher, int dtype, int64_t n, float alpha, float eps,
                    void* out, void* stream);
/* batched form: host arrays [batch] of device pointers (fisher_host may be NULL or hold NULL entries); one call for the
 * q/k/v/o (gate/up) Linears of a layer or a whole same-shape batch of asvd_svd_batched.  Asynchronous. */
int asvd_make_scale_batched(int batch, const void* const* scaling_host, const void* const* fisher_host, int dtype, int64_t n,
                            float alpha, float eps, void* const* out_host, void* stream);

/* K3b  w_scaled[i][j] = float(w[i][j]) * float(s[j]).  Replaces svd_linear.py:47,60
 * (`w = linear.weight.data.float(); w = w * scaling_diag_matrix.view(1,-1)`).  s may be NULL (plain
 * upcast).  Stand-alone form used by parity tests; asvd_svd fuses the same arithmetic into its pack
 * kernel.  Asynchronous. */
int asvd_scale_cols(const void* w, int w_dtype, int64_t m, int64_t n, int64_t ldw,
                    const void* s, int s_dtype, float* out, int64_t ldo, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K4  economy SVD in fp32:   A * diag(col_scale) = U diag(S) V^T .
 * Replaces the factorisation call at svd_linear.py:65 (`torch.svd_lowrank(w, q=rank)`; the parity
 * oracle named by BASELINE.json is the exact `torch.linalg.svd(w, full_matrices=False)`), and, with
 * U = V = NULL, the values-only `torch.svd(w.float(), compute_uv=False)` at sensitivity.py:101.
 *
 * Algorithm: the oriented matrix (rows >= cols) is reduced to a square one by a Cholesky-QR in fp64 (Gram matrix
 * by fp64 MFMA, columns ordered by norm), then one-sided block Jacobi runs on R^T: XOR pair schedule over 32-column panels
 * (panel counts that are not a power of two: a grouped schedule — XOR inside groups of 2..16 super-panels, round-robin over
 * the groups); dense sweeps work on 64-column super-panels, TWO launches per super-step: the wave-local 64x64 eigen-solves
 * (one wave per solve, the matrix in registers, both inner steps of a super-pair; from 2048 columns on the second inner step visits
 * only the cross pairs of its two panels, on a ring of interleaved positions: half the phases) and one 128-wide update pass fused with the
 * Gram tiles of the next step, in split-fp16 arithmetic (three products per fp32 product, power-of-two column scales from the
 * carried column norms; a problem that turns NaN on that path is repeated with the separate fp32 Gram / split-bf16 update
 * passes); tail sweeps rotate only the pairs a blocked X^T X snapshot marks.  Right vectors are the rotated columns, left
 * vectors X V by one GEMM, sigma_j = |X v_j| in fp64.  No vector is accumulated during the sweeps.  Problems too small or
 * rank-deficient for the reduction take the same sweeps on the matrix itself.
 *
 *   batch       number of same-shape problems solved concurrently (fills the 256 CUs)
 *   a_host      host array [batch] of device pointers to A_b  [m, n] row-major, leading dim lda
 *   cs_host     host array [batch] of device pointers to column scales s_b [n] (or NULL / NULL entries)
 *   U_host      host array [batch] of device pointers to U_b [m, k] row-major (NULL: no vectors)
 *   S_host      host array [batch] of device pointers to S_b [k] descending
 *   V_host      host array [batch] of device pointers to V_b [n, k] row-major (NULL: no vectors)
 *   k           number of leading singular triplets to write, 1 <= k <= min(m, n).  The stopping rule (tol) looks only at the
 *               kb = min(ceil(k / 32) + 1, panels) leading 32-column panels (those holding the k leading columns plus one panel of
 *               margin): with k < min(m,n) the sweeps stop as soon as that part is done (the discarded tail converges last and would
 *               cost 2-4 more sweeps).  The finalisation still ranks ALL columns by norm and writes the k largest.  What a call with
 *               k < min(m, n) guarantees (tests/test_gpu_svd_topk.py): the contract of a full call on its k triplets — sigma within
 *               1e-4 of the exact spectrum, orthonormal vectors, and at every rank r <= k a rank-r reconstruction whose error is the
 *               optimal (Eckart-Young) one to 1e-3 |A diag(s)|_F — no more sweeps than the full call, and the leading k values and
 *               every rank-r slice equal to the full call's to 2e-6 sigma_1 / 1e-4 relative
 *   max_sweeps  <=0: default (30)
 *   tol         <=0: default (1e-6).  Bound on the stopping measure: max |g_ij| / max(g_ii, g_jj) over the column pairs (i, j) that
 *               touch one of the kb leading panels (g = X^T X of the working columns).  The cosine |g_ij| / sqrt(g_ii g_jj) only
 *               decides which pairs rotate and which pairs the snapshots of the sparse sweeps mark
 *   info_host   optional host int[4*batch]: {status, sweeps, rotated pairs in last sweep, float bits of the last sweep's stopping measure}
 * Host-synchronous: the call returns when S/U/V are complete.  Sync points (csrc/svd_jacobi.hip): one after the reduction
 * (Cholesky breakdown flag), one per Jacobi sweep (convergence flags: four ints per problem), one more per sparse sweep
 * (the pair marks of the coupling snapshot go to the host, which packs them into rounds of disjoint pairs), one when a
 * problem finishes early (its `done` flag goes to the device), one at the end — 13 for a 4096 x 4096 call, 0.3 % of its time.
 * Everything is enqueued on `stream`; the one exception is the split of a large batch over two internal CU-masked streams
 * (asvd_svd_set_split below: what the library OWNS for it and when it refuses; the streams wait for everything queued on `stream` before the
 * call, and the call returns synchronised).  Concurrent calls from
 * different host threads on different streams and workspaces are safe: no shared mutable state — schedule tables and modes
 * travel by value in the kernel arguments, not in __constant__ memory; the profiling counters are per thread — and no kernel
 * uses scratch.  tests/test_gpu_concurrency.py holds the library to it (two threads x 8 x 4096^2 next to a stream of foreign
 * GEMMs, and calls with different pair schedules side by side: bit-identical results and sweep counts against serial runs).
 * Environment (read on the host, all optional; none changes results beyond rounding): ASVD_DEBUG (trace on stderr),
 * ASVD_SUPGRAM=0 (separate Gram / update passes), ASVD_NO_REDUCE (skip the Cholesky-QR), ASVD_EVDQ=0/1 (force the throughput / latency form of
 * the eigen-solver), ASVD_SPLIT=0 (never split a batch over the two halves of the chip), ASVD_RING=2 (cross-only ring visit of inner step 1 of
 * the eigen-solves below 2048 columns too; the default from 2048 columns on), ASVD_GRAM_I8=0 (Gram matrix of the reduction with the fp64 matrix
 * instructions instead of the exact int8 digit products, csrc/gram_i8.h), ASVD_NN_I8=0 (long-side product X V with six bf16 products per fp32
 * product instead of the int8 fixed-point form, csrc/nn_gemm_i8.h), ASVD_SNAP_I8=0 (coupling snapshot of the sparse sweeps with three fp16
 * products per fp32 product instead of int8 digit planes, csrc/snapshot_i8.h).
 * Returns worst status over the batch.
 */
int asvd_svd_worksize(int batch, int64_t m, int64_t n, int want_vectors, size_t* bytes);
int asvd_svd_batched(int batch, const void* const* a_host, int a_dtype, int64_t m, int64_t n, int64_t lda,
                     const void* const* cs_host, int cs_dtype,
                     float* const* U_host, float* const* S_host, float* const* V_host, int64_t k,
                     int max_sweeps, float tol, void* work, size_t work_bytes, int* info_host, void* stream);
/* Which path the last asvd_svd_batched / asvd_svd call of THIS host thread took: an OR of the bits below over the problems of the batch (both
 * halves of a split batch).  The results meet the same contract on every path; the bits are there so that a caller — and the parity tests —
 * can tell a silent change of arithmetic from the default one. */
#define ASVD_PATH_REDUCED 1          /* Cholesky-QR reduction + Jacobi on R^T (the default for >= 128 columns) ran to completion */
#define ASVD_PATH_REDUCE_FALLBACK 2  /* the Cholesky broke down (pivot <= 1e-13: numerically rank-deficient) -> the whole call ran the direct path */
#define ASVD_PATH_PLAIN_RETRY 4      /* a problem turned NaN in the split-fp16 fused kernel -> the sweeps were repeated with the separate passes */
#define ASVD_PATH_SPLIT 8            /* the batch ran as two halves on two CU-masked streams */
#define ASVD_PATH_SPLIT_REFUSED 16   /* the batch qualified for the split but ran as one call on the caller's stream: another process computes on the
                                        device or the caller's stream carries a CU mask of its own */
#define ASVD_PATH_GRAM_RETRY 32      /* the Cholesky broke down on the int8 Gram matrix (columns rounded to 2^-25 of their largest entry) and the reduction was
                                      * repeated with the fp64 Gram matrix of the exact columns (which either completes: REDUCED, or breaks down too: REDUCE_FALLBACK) */
int asvd_svd_get_last_path(void);
/* single-problem convenience wrapper (batch = 1) */
int asvd_svd(const void* a, int a_dtype, int64_t m, int64_t n, int64_t lda, const void* col_scale, int cs_dtype,
             float* U, float* S, float* V, int64_t k, int max_sweeps, float tol,
             void* work, size_t work_bytes, int* info_host, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K4s  largest singular value only.  Replaces sensitivity.py:101-102 of calib_sensitivity_stable_rank
 * (`_, singular_values, _ = torch.svd(w.float(), compute_uv=False); spectral_norm = torch.max(singular_values)`):
 * the reference factorises the whole matrix and keeps one number.  Lanczos on W^T W (two matrix-vector passes
 * over W per step, fp32 vectors, fp64 recurrence coefficients); every 16 steps the largest Ritz value is found by
 * multisection on the Sturm count and the iteration stops when it moved by less than tol (relative, in sigma^2)
 * over the last 16 steps.  HBM/L2-bound: 2*m*n*sizeof(elem) bytes per step.
 *   a_host      host array [batch] of device pointers to W_b [m, n] row-major (leading dim lda), n <= 16384
 *   sigma_host  host array [batch] of device pointers to one float each (sigma_max of W_b)
 *   max_steps   <=0: default 1024 (rounded up to a multiple of 16);  tol <=0: default 1e-8
 *   info_host   optional host int[2*batch]: {status, Lanczos steps}
 * Host-synchronous (one stream sync per 16 steps).  Returns worst status over the batch (ASVD_N_NOCONV: value is a
 * lower bound that was still moving — callers fall back to asvd_svd_batched with k = 1).
 */
int asvd_sigma_max_worksize(int batch, int64_t m, int64_t n, int max_steps, size_t* bytes);
int asvd_sigma_max_batched(int batch, const void* const* a_host, int a_dtype, int64_t m, int64_t n, int64_t lda,
                           float* const* sigma_host, int max_steps, float tol, void* work, size_t work_bytes,
                           int* info_host, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K18  re-orthonormalise columns in their given order (new; the reference gets an orthonormal basis from the QR inside torch.svd_lowrank).
 * The SVD above returns the short side's vectors orthonormal to 1e-5 but the long side's from one product u_j = A v_j / sigma_j, whose defect
 * grows with sigma_1 / sigma_j.  This is the opt-in repair, a post-pass on finished output; nothing above calls it.
 * One pass:  E = Q^T Q - I,  T = striu(E) + diag(E) / 2,  Q <- Q - Q T  (first-order inverse of the Cholesky factor of Q^T Q: every pass multiplies
 * Q from the right by an upper-triangular matrix with positive diagonal, so span(q_1..q_j) is kept for every j and the limit is the Cholesky-QR
 * factor of the input).  Passes repeat until max |E| <= tol; the final max |E| is measured by a last Gram pass (p passes cost p + 1 Gram passes).
 * E is the exact Gram matrix of the columns rounded to 24-bit fixed point (int8 digit products, fp64 combination, identity subtracted before the
 * rounding to fp32; for m > 32768 the row segments of 32768 are added in fp32); the update runs on the fp32 matrix instructions, in place.
 *   Q_host      host array [batch] of device pointers to Q_b [m, k] fp32 row-major, leading dim ldq >= k, m >= k >= 1 (any k, any ldq; 4-byte
 *               aligned); columns [k, ldq) are neither read nor written
 *   max_passes  <=0: default (8);   tol  <=0: default (2e-6)
 *   info_host   optional host int[4*batch]: {status, passes, float bits of max |E| at entry, float bits of max |E| measured at exit}
 * Per problem: entry max |E| non-finite -> ASVD_N_NAN, Q_b untouched; entry max |E| > 0.25 (the iteration is not monotone and diverges from about
 * 1; a zero column gives E_jj = -1) -> ASVD_N_NOCONV, Q_b untouched; a value >= 1 or non-finite inside the loop, or max_passes reached with
 * max |E| > tol -> ASVD_N_NOCONV.  One problem's refusal does not touch the others: every problem's arithmetic is its own, so its bits equal
 * those of a call without the refused one.  Two calls on equal input give equal bits.
 * Host-synchronous: one stream synchronisation per Gram pass.  The batch runs in sub-batches that keep the workspace at or under 1 GiB (one
 * problem at a time when one alone needs more): 32 x 4096 x 4096 runs 9 problems at a time in 1008 MiB (per problem: 48 MiB digit planes + 64 MiB T);
 * 32 x 4096 x 1843 runs 28 at a time in 1003 MiB (35.8 MiB per problem).
 * Returns worst status over the batch; bad arguments (NULL, batch < 1, k < 1, m < k, ldq < k, misaligned Q) return ASVD_E_BADARG before any device
 * call, a short workspace ASVD_E_WORKSPACE. */
int asvd_reorth_worksize(int batch, int64_t m, int64_t k, size_t* bytes);
int asvd_reorth_batched(int batch, float* const* Q_host, int64_t m, int64_t k, int64_t ldq, int max_passes, float tol, void* work,
                        size_t work_bytes, int* info_host, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K5/K6  truncate to rank r, un-scale V, fuse sigma, transpose V, down-cast, NaN flag.
 * Replaces svd_linear.py:69-70 (`V = V / s.view(-1,1)`), :81-98 (NaN checks) and SVDLinear.__init__
 * :16-24 + the `.to(dtype)` at :102:
 *   UV: A = U[:, :r] * sqrt(S[:r])           B = (V[:, :r] / s[:,None]).T * sqrt(S[:r])[:,None]
 *   U : A = U[:, :r] * S[:r]                 B = (V[:, :r] / s[:,None]).T
 *   V : A = U[:, :r]                         B = (V[:, :r] / s[:,None]).T * S[:r][:,None]
 * all in fp32, then rounded once (RNE) to out_dtype.
 *   U [m, ldu>=r], S [>=r], V [n, ldv>=r] fp32;  s [n] in s_dtype or NULL;
 *   A [m, r] (ALinear.weight), B [r, n] (BLinear.weight) contiguous in out_dtype;
 *   nan_flags: device int[3] OR-ed with 1 where S / U / V hold a NaN within the first r columns
 *              (caller zero-initialises; NULL to skip).  Asynchronous.
 */
int asvd_truncate_split(const float* U, int64_t ldu, const float* S, const float* V, int64_t ldv,
                        const void* s, int s_dtype, int64_t m, int64_t n, int64_t r, int sigma_fuse,
                        void* A, void* B, int out_dtype, int* nan_flags, void* stream);
/* batched form over same-shape problems: host arrays [batch] of device pointers; nan_flags: device int[3 * batch] (3 per
 * problem, caller zero-initialises) or NULL.  Asynchronous. */
int asvd_truncate_split_batched(int batch, const float* const* U_host, int64_t ldu, const float* const* S_host,
                                const float* const* V_host, int64_t ldv, const void* const* s_host, int s_dtype, int64_t m,
                                int64_t n, int64_t r, int sigma_fuse, void* const* A_host, void* const* B_host, int out_dtype,
                                int* nan_flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K8  squared Frobenius norm (sensitivity.py:100 `torch.norm(w, p="fro") ** 2`), fp32 accumulate in
 * fixed order, result written to *out (device float).  work: asvd_fro_worksize bytes.  Asynchronous. */
int asvd_fro_worksize(int64_t m, int64_t n, size_t* bytes);
int asvd_fro_norm_sq(const void* w, int w_dtype, int64_t m, int64_t n, int64_t ldw, float* out,
                     void* work, size_t work_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K9  parity evidence (new; no reference counterpart — BASELINE.json north_star "reconstructed W <= 1e-3 Frobenius"):
 *        err2 = |W - A*B|_F^2 , w2 = |W|_F^2      (A, B = ALinear.weight, BLinear.weight of an SVDLinear: svd_linear.py:8-24)
 *   W [m, n] in w_dtype (ldw), A [m, r], B [r, n] contiguous in ab_dtype.  F16 / BF16 factors: tiled GEMM on the fp16 / bf16 matrix pipe
 *   (products of 16-bit factors are exact there, fp32 accumulation) fused with the squared-difference reduction in fp64, 2 m n r flop.  When
 *   n % 8 == 0 and B is 16-byte aligned (every Linear of the models this path serves) the GEMM reads the factors AS STORED — A rows at any 2-byte
 *   alignment (odd ranks), B transposed on its way into LDS: ONE GEMM launch + the ordered sum of its partials; A is read in aligned 4-byte words, so
 *   its allocation must be readable up to the next 4-byte boundary.  Otherwise: zero-padded K-contiguous copies in the workspace first (two more
 *   launches).  F32 factors: fp32 MFMA, one wave per 32x32 tile.  out: device double[2] = {err2, w2}.  work: asvd_reconstruct_worksize(m, n, r)
 *   bytes (partial sums + room for the padded copies).  Asynchronous. */
int asvd_reconstruct_worksize(int64_t m, int64_t n, int64_t r, size_t* bytes);
int asvd_reconstruct_err(const void* W, int w_dtype, int64_t ldw, const void* A, const void* B, int ab_dtype,
                         int64_t m, int64_t n, int64_t r, double* out, void* work, size_t work_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K10  fused SVDLinear forward for few tokens (modules/svd_linear.py:105-109 `y = self.BLinear(inp); y = self.ALinear(y)`):
 *        y[T, N] = fp16( fp16(x Bp^T) Ap^T + bias )
 *   ONE persistent launch (phase 1 z = x Bp^T, in-kernel grid barrier, phase 2 y = z Ap^T + bias); the r-wide intermediate z is
 *   rounded to fp16 exactly where BLinear's output is, lives in `work` (agent-scope stores / loads, no cache-wide fence) and is
 *   consumed inside the launch; B and A cross HBM once.  T <= 4: a pair of fused GEMVs (v_dot2_f32_f16); larger T: fp16 MFMA tiles.
 *   x [T, K] fp16 contiguous, 1 <= T <= ASVD_LOWRANK_MAX_TOKENS;  K % 64 == 0;
 *   Bp [rp, K] = BLinear.weight [r, K] with zero rows appended, Ap [N, rp] = ALinear.weight [N, r] with zero columns appended,
 *   rp = asvd_lowrank_padded_rank(r) (multiple of 64);  bias [N] fp16 or NULL;  y [T, N] fp16 contiguous.
 *   work: asvd_lowrank_work_bytes(T, rp) bytes, 16-byte aligned, whose first 256 bytes the caller zeroes ONCE (barrier state; the
 *   kernel leaves them reusable); one `work` must not be used by two launches in flight at the same time.  Asynchronous.
 *   For larger T the reference's two GEMMs are the right shape (weights amortised over tokens); this entry refuses them. */
#define ASVD_LOWRANK_MAX_TOKENS 256
int64_t asvd_lowrank_padded_rank(int64_t r);
size_t asvd_lowrank_work_bytes(int64_t T, int64_t rp);
int asvd_lowrank_forward_f16(const void* x, int64_t T, const void* Bp, const void* Ap, const void* bias, int64_t N, int64_t K,
                             int64_t rp, void* y, void* work, size_t work_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K11  round-to-nearest weight quantization (fake quantization: the weight keeps its dtype).  Replaces quantization.py:17-21,31-145
 * (Quantizer.configure(bits, perchannel=True, sym=False, mse=False); find_params(W.float(), weight=True); quantize) as
 * rtn_quant_sequential (:157-175) applies it to every nn.Linear of the decoder blocks.  Per row of W, in fp32:
 *   xmin = min(min(row), 0)   xmax = max(max(row), 0)   (both 0: -1 and +1)   maxq = 2^bits - 1
 *   scale = (xmax - xmin) / maxq    zero = round(-xmin / scale)    q = clamp(round(x / scale) + zero, 0, maxq)
 *   out = scale * (q - zero), rounded once (RNE) to the weight dtype.
 * Bit for bit the reference's torch sequence: IEEE fp32 division, round half to even, fp32 denormals kept, NaN-propagating min / max /
 * clamp (a row holding a NaN or an Inf comes out all NaN, as in torch).  One read and one write of W per row.
 *   W [rows, cols] in dtype (F32 / F16 / BF16), leading dimension ldw;  out [rows, cols] in the same dtype, ldo; out may be W itself.
 *   bits in 1..8.  scale, zero: device float[rows] or NULL;  codes: device uint8 [rows, cols] contiguous (q) or NULL (NaN q -> 0).
 *   flag: device int, caller-zeroed, OR-ed with 1 when some row's scale is 0 (fp32 rows whose values are all of denormal size): the
 *         reference then returns the tensor UNCHANGED (Quantizer.ready()), so the caller must keep W and discard out.  Such rows are
 *         copied to out unchanged, the others are quantized, so with out == W a flagged tensor is partly quantized: pass a separate out
 *         when W may hold such rows.  Asynchronous.
 * Batched form: one launch per 16 tensors of mixed shapes, strides and dtypes; host arrays [batch] (w_host, dtype_host, rows_host,
 * cols_host, ldw_host, out_host, ldo_host; scale_host / zero_host / codes_host may be NULL or hold NULL entries); flags: device
 * int[batch], caller-zeroed, one per tensor. */
int asvd_rtn_quant(const void* w, int dtype, int64_t rows, int64_t cols, int64_t ldw, int bits, void* out, int64_t ldo, float* scale,
                   float* zero, void* codes, int* flag, void* stream);
int asvd_rtn_quant_batched(int batch, const void* const* w_host, const int* dtype_host, const int64_t* rows_host, const int64_t* cols_host,
                           const int64_t* ldw_host, int bits, void* const* out_host, const int64_t* ldo_host, float* const* scale_host,
                           float* const* zero_host, void* const* codes_host, int* flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K12  RTN-quantized weights kept as uint8 codes (the q / scale / zero of K11): forward and dequantization.
 *   w[n, k] = scale[n] * (float(q[n, k]) - zero[n]), evaluated in fp32 (the subtraction is exact) and rounded once (RNE) to the weight dtype:
 *   bit for bit the `out` of asvd_rtn_quant for the same codes.
 * asvd_w8_linear_f16:  y[T, N] = fp16( x[T, K] . w^T + bias ) with w dequantized to fp16 in registers, fp32 accumulation on the fp16 matrix
 *   pipe and one rounding at the end: nn.Linear on the fake-quantized weight up to the order of the fp32 sums.  One launch; the k range is split
 *   over the waves of a workgroup and summed in a fixed order (no atomics, nothing crosses workgroups): two calls give identical bits.
 *   x [T, K] fp16 contiguous, 1 <= T <= ASVD_W8_MAX_TOKENS (asvd_w8_linear_max_tokens() returns it);  q [N, ldq] uint8, ldq >= K;  scale, zero
 *   [N] fp32;  bias [N] fp16 or NULL;  y [T, N] fp16 contiguous;  any K >= 1, any N >= 1.  Rows are streamed with 16-byte loads when x and q are
 *   16-byte aligned, K % 8 == 0 and ldq % 16 == 0 (element loads for the last K % 16 codes, and throughout otherwise).  The element-load form is correct but slow (measured 3.3-3.7x the time
 *   of an fp16 GEMM at K = 1843): callers that care about speed send such layers through asvd_w8_dequant + their GEMM.  x, y and bias must be 2-byte aligned.
 *   An SVDLinear with packed factors is two calls (z, then y), or one of K16.  Asynchronous.
 * asvd_w8_dequant:  out [rows, cols] (ldo) in out_dtype (F32 / F16 / BF16) from q [rows, ldq], scale, zero [rows].  Asynchronous.
 * Bad arguments (NULL, T out of range, ldq < K, misaligned x / y / out) return ASVD_E_BADARG before any device call. */
#define ASVD_W8_MAX_TOKENS 256
int64_t asvd_w8_linear_max_tokens(void);
int asvd_w8_linear_f16(const void* x, int64_t T, const void* q, int64_t ldq, const float* scale, const float* zero, const void* bias,
                       int64_t N, int64_t K, void* y, void* stream);
int asvd_w8_dequant(const void* q, int64_t ldq, const float* scale, const float* zero, int64_t rows, int64_t cols, void* out, int out_dtype,
                    int64_t ldo, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K13  The codes of K11 stored at their own width, bits = 6 or 4 (the quantizer's range 0 .. 2^bits - 1 needs no more).
 * Format ("bitstream64", an on-disk format): a row of K codes is a little-endian bitstream, code k in bits [bits k, bits (k + 1)) of the row
 *   read as one little-endian integer, zero-padded to whole blocks of 64 codes.  A block is 8 bits bytes (48 at 6 bits, 32 at 4), a row
 *   asvd_wb_row_bytes(K, bits) = ceil(K / 64) * 8 * bits bytes: a multiple of 16, so with a 16-byte-aligned base and leading dimension every
 *   block starts 16-byte aligned.  At 6 bits codes 5 and 10 of every 16 cross a 32-bit word, at 4 bits none does.  Padding codes are 0 and never
 *   part of the weight.
 * asvd_wb_row_bytes:  host-only query; -1 for bits other than 4 and 6 or cols < 1.
 * asvd_wb_pack:  q [rows, ldq] uint8 codes (ldq >= cols) -> out [rows, ld_bytes] bitstream rows (ld_bytes >= row bytes; out and ld_bytes multiples
 *   of 4).  Codes are masked to `bits` bits (the quantizer emits none beyond).  Bytes of a row beyond its row bytes are not written.  Asynchronous.
 * asvd_wb_dequant:  out [rows, cols] (ldo) in out_dtype (F32 / F16 / BF16) from the bitstream rows q (q and ld_bytes multiples of 4), value for
 *   value asvd_w8_dequant on the unpacked codes: fp32 subtraction, one fp32 product, one rounding.  Any cols >= 1, any destination aligned to its
 *   element; nothing outside [rows, cols] is written.  Asynchronous.
 * asvd_wb_linear_f16:  asvd_w8_linear_f16 on bitstream rows: the same tiles, the same split of k over the waves, the same order of every sum,
 *   the codes cut out of three (6 bits) or two (4 bits) 16-byte loads per lane and iteration instead of four.  The result has the BITS of
 *   asvd_w8_linear_f16 on the same codes, scale, zero and bias.  K % 16 == 0 only; x, q and ld_bytes 16-byte aligned; y and bias 2-byte aligned;
 *   1 <= T <= ASVD_W8_MAX_TOKENS.  Asynchronous.
 * Bad arguments (NULL, other widths, T out of range, K % 16 != 0, short leading dimensions, misaligned x / q / y / out) return ASVD_E_BADARG
 * before any device call. */
int64_t asvd_wb_row_bytes(int64_t cols, int bits);
int asvd_wb_pack(const void* q, int64_t ldq, int64_t rows, int64_t cols, int bits, void* out, int64_t ld_bytes, void* stream);
int asvd_wb_dequant(const void* q, int64_t ld_bytes, int bits, const float* scale, const float* zero, int64_t rows, int64_t cols, void* out,
                    int out_dtype, int64_t ldo, void* stream);
int asvd_wb_linear_f16(const void* x, int64_t T, const void* q, int64_t ld_bytes, int bits, const float* scale, const float* zero,
                       const void* bias, int64_t N, int64_t K, void* y, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K14  Group-wise RTN: one scale and one zero per group of G = 64 or 128 consecutive columns of a row instead of per row.  A row of K columns
 *   has ng = ceil(K / G) groups; the last one holds K - (ng - 1) G columns when K is no multiple of G.  Group j of row n is quantized exactly as
 *   K11 quantizes the one-row tensor W[n, jG : (j+1)G] (min / max including 0, -1 / +1 for an all-zero group, fp32 division, round half to even,
 *   NaN-propagating min / max: a NaN poisons its own group only).  scale, zero: device float [rows, ng], row-major, contiguous.
 *   `group` must be 64 or 128 in every entry below (per-row scales are the K11 - K13 entries); anything else returns ASVD_E_BADARG.
 * asvd_rtn_quant_grouped, asvd_rtn_quant_grouped_batched:  asvd_rtn_quant / asvd_rtn_quant_batched with `group` as last argument.  The flag is
 *   OR-ed with 1 when some GROUP's scale is 0 (the reference's Quantizer.ready() over the tensor reshaped to groups); such groups are copied.
 * asvd_w8_linear_grouped_f16, asvd_wb_linear_grouped_f16:  the forwards of K12 / K13 with w[n, k] = fp16(scale[n, k / G] * (code - zero[n, k / G])),
 *   formed in registers before the matrix instruction as there; the same tiles, k split and order of sums, so with every group of a row given
 *   one scale and zero the result has the bits of the per-row entry, and the 6- and 4-bit forms give the bits of the 8-bit form on the same
 *   codes.  At all three widths: K % 16 == 0, x and q 16-byte aligned, the leading dimension a multiple of 16.
 * asvd_w8_dequant_grouped, asvd_wb_dequant_grouped:  the dense weight, bit for bit the `out` of the grouped quantizer; arguments as their
 *   per-row siblings.
 * Bad arguments return ASVD_E_BADARG before any device call. */
int asvd_rtn_quant_grouped(const void* w, int dtype, int64_t rows, int64_t cols, int64_t ldw, int bits, void* out, int64_t ldo, float* scale,
                           float* zero, void* codes, int* flag, void* stream, int64_t group);
int asvd_rtn_quant_grouped_batched(int batch, const void* const* w_host, const int* dtype_host, const int64_t* rows_host,
                                   const int64_t* cols_host, const int64_t* ldw_host, int bits, void* const* out_host, const int64_t* ldo_host,
                                   float* const* scale_host, float* const* zero_host, void* const* codes_host, int* flags, void* stream,
                                   int64_t group);
int asvd_w8_linear_grouped_f16(const void* x, int64_t T, const void* q, int64_t ldq, const float* scale, const float* zero, int64_t group,
                               const void* bias, int64_t N, int64_t K, void* y, void* stream);
int asvd_w8_dequant_grouped(const void* q, int64_t ldq, const float* scale, const float* zero, int64_t group, int64_t rows, int64_t cols,
                            void* out, int out_dtype, int64_t ldo, void* stream);
int asvd_wb_dequant_grouped(const void* q, int64_t ld_bytes, int bits, const float* scale, const float* zero, int64_t group, int64_t rows,
                            int64_t cols, void* out, int out_dtype, int64_t ldo, void* stream);
int asvd_wb_linear_grouped_f16(const void* x, int64_t T, const void* q, int64_t ld_bytes, int bits, const float* scale, const float* zero,
                               int64_t group, const void* bias, int64_t N, int64_t K, void* y, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K15  RTN with the clip search of the reference's Quantizer (quantization.py:94-111, mse=True).  A unit is a row (group 0) or a group of 64 / 128
 *   columns.  Its base pair (scale, zero) is that of K11 / K14.  Candidate i = 0 .. n - 1, n = int(maxshrink * grid) as Python computes it in
 *   double, shrinks the range: p = float(1 - i / grid) (double arithmetic, one cast), xmin1 = p xmin, xmax1 = p xmax,
 *   scale1 = (xmax1 - xmin1) / maxq, zero1 = rint(-xmin1 / scale1), each operation rounded to fp32 on its own.  The pair kept is the one with
 *   the smallest sum over the unit of |scale1 (clamp(rint(x / scale1) + zero1, 0, maxq) - zero1) - x|^norm; a candidate replaces the best so far
 *   only when its sum is strictly smaller, so the lowest index wins ties and a NaN or infinite sum never wins.  A unit whose base scale is 0,
 *   infinite or NaN keeps its base pair and is flagged or poisoned as without the search.  The sums are evaluated with a hardware reciprocal,
 *   exp2(norm log2|d|) and a fixed order of additions: the choice among near-tied candidates may differ from an fp64 evaluation by that much,
 *   and two calls give the same bits.  out, codes, scale and zero are then written as by K11 / K14 with the chosen pair, in the same arithmetic.
 * asvd_rtn_quant_mse_batched:  the arguments of asvd_rtn_quant_grouped_batched (group 0, 64 or 128), then the search's norm (2.4 in the
 *   reference), grid (100) and maxshrink (0.8).  ASVD_E_BADARG before any device call for norm <= 0 or not finite, grid < 1, maxshrink outside
 *   (0, 1], or a candidate count outside 1 .. 256.  maxshrink is read as the shortest decimal that gives that float (0.7f counts as 0.7). */
int asvd_rtn_quant_mse_batched(int batch, const void* const* w_host, const int* dtype_host, const int64_t* rows_host, const int64_t* cols_host,
                               const int64_t* ldw_host, int bits, void* const* out_host, const int64_t* ldo_host, float* const* scale_host,
                               float* const* zero_host, void* const* codes_host, int* flags, void* stream, int64_t group, float norm, int grid,
                               float maxshrink);

/* ---------------------------------------------------------------------------------------------
 * K16  A packed SVDLinear factor pair (K12 - K14 codes on both factors) in ONE launch, for decode-sized inputs:
 *        z[T, r] = fp16( x[T, K] . wB^T )      y[T, N] = fp16( z . wA^T + bias )
 *   with wB / wA dequantized in registers as in K12 - K14.  One persistent launch of at most one workgroup per CU: phase 1 (z), the in-kernel
 *   grid barrier of K10, phase 2 (y).  Both phases run the tile routine of asvd_w8_linear*_f16 / asvd_wb_linear*_f16, so the result has the
 *   BITS of those two calls (z, then y) on the same buffers.  It reads the factors' own code / scale / zero buffers: no padded copies.
 *   x [T, K] fp16 contiguous, 1 <= T <= ASVD_W8_MAX_TOKENS;  K % 16 == 0, r % 16 == 0;  y [T, N] fp16 contiguous;  bias [N] fp16 or NULL.
 *   bits: the STORAGE width of both factors: 8 (one code per byte, ld >= columns), 6 or 4 (bitstream64 rows, ld >= asvd_wb_row_bytes).
 *   qB: r rows of K codes, ldB bytes apart;  qA: N rows of r codes, ldA bytes apart.  group: 0 (scaleB, zeroB [r]; scaleA, zeroA [N]) or
 *   64 / 128 ([r, ceil(K / group)]; [N, ceil(r / group)]), the same for both factors.  x, qB, qA and work 16-byte aligned, ldB and ldA
 *   multiples of 16, y and bias 2-byte aligned.
 *   work: asvd_lowrank_packed_work_bytes(T, r) = 256 + round_up(T, 32) * r * 2 bytes (a host-side query), whose first 256 bytes the caller
 *   zeroes ONCE (barrier state, reusable; the rest needs no initialisation); one `work` must not be used by two launches in flight at the same
 *   time.  As in K10 the launch assumes its workgroups co-resident; one that waits too long at the barrier sets word 2 of `work` (sticky, the
 *   host clears it) and every workgroup then overwrites what it stored of y with NaN: such a launch never hangs and never returns numbers.
 *   Asynchronous.  Bad arguments (NULL other than bias, T out of range, other widths or group sizes, K % 16 or r % 16 != 0, short or
 *   misaligned leading dimensions, misaligned pointers) return ASVD_E_BADARG, a short workspace ASVD_E_WORKSPACE, before any device call. */
size_t asvd_lowrank_packed_work_bytes(int64_t T, int64_t r);
int asvd_lowrank_packed_f16(const void* x, int64_t T, const void* qB, int64_t ldB, const float* scaleB, const float* zeroB, const void* qA,
                            int64_t ldA, const float* scaleA, const float* zeroA, int bits, int64_t group, const void* bias, int64_t N,
                            int64_t K, int64_t r, void* y, void* work, size_t work_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K17  A token-tiled GEMM on packed RTN codes, for inputs beyond decode (prefill, perplexity windows, batched decode):
 *        y[T, N] = fp16( x[T, K] . w^T + bias ),   w[n, k] = fp16( scale * (code - zero) )
 *   ONE entry for what K12 / K13 / K14 cover in four.  w is formed in registers, bit for bit what asvd_w8_dequant / asvd_wb_dequant write (the
 *   subtraction, one fp32 product, one rounding; the scale never moves behind the accumulation), and goes to the fp16 matrix instruction with
 *   fp32 accumulation.  A workgroup owns 32 m tokens x 32 m features (m = 4, 2 or 1, chosen from T, N and the CU count), stages its x tile once
 *   per 128 (4 / m) values of k through LDS for all its waves, and streams each code once per 32 m tokens.  Every sum has a fixed order (no atomics):
 *   two calls return the same bits; the order depends on (T, N, CU count) only.  A token row depends on its own x row only: beyond T, N and K
 *   nothing that exists is multiplied by padding, so a NaN / Inf in one token row changes that row only.
 *   x [T, K] fp16 contiguous, 1 <= T <= ASVD_PACKED_GEMM_MAX_TOKENS (asvd_packed_gemm_max_tokens() returns it);  y [T, N] fp16 contiguous;
 *   bias [N] fp16 or NULL.  bits: the STORAGE width: 8 (q [N, ld_bytes], one code per byte, ld_bytes >= K) or 6 / 4 (bitstream64 rows of
 *   asvd_wb_row_bytes(K, bits) bytes, ld_bytes apart).  group: 0 (scale, zero [N]) or 64 / 128 ([N, ceil(K / group)]).  K % 16 == 0;  x and q
 *   16-byte aligned, ld_bytes a multiple of 16;  y and bias 2-byte aligned.  No workspace.  Asynchronous.
 *   Bad arguments (NULL other than bias, T out of range, other widths or group sizes, K % 16 != 0, a short or misaligned ld_bytes, misaligned
 *   pointers) return ASVD_E_BADARG before any device call. */
#define ASVD_PACKED_GEMM_MAX_TOKENS 1048576
int64_t asvd_packed_gemm_max_tokens(void);
int asvd_packed_gemm_f16(const void* x, int64_t T, const void* q, int64_t ld_bytes, int bits, const float* scale, const float* zero, int64_t group,
                         const void* bias, int64_t N, int64_t K, void* y, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K19  bf16 activations on the packed-weight kernels: K12 / K13 / K14, K16 and K17 with the activation dtype and the group size as arguments.
 *   act_dtype: ASVD_F16 or ASVD_BF16, the type of x, bias, y (and of the intermediate z of the pair) AND of the weight the codes stand for:
 *        y[T, N] = act( x[T, K] . w^T + bias ),   w[n, k] = act( scale * (code - zero) )
 *   Anything else (ASVD_F32 included) returns ASVD_E_BADARG before any device call.  With ASVD_F16 every entry IS its _f16 counterpart (those
 *   forward here) and returns its bits.  With ASVD_BF16 the kernels differ in four places and nowhere else: w is the fp32 value rounded ONCE
 *   (RNE) to bf16, the bits asvd_w8_dequant / asvd_wb_dequant write with out_dtype ASVD_BF16 for finite values; the matrix instruction is the
 *   bf16 one on the same operands (the same tiles, k permutation, split of k over the waves and order of every fp32 sum); the bias is read
 *   as bf16; y (and z) are rounded RNE to bf16.  A pair that gives up at its barrier overwrites y with bf16 NaNs.
 *   group: 0 (scale, zero per row), 64 or 128 (per group of that many columns), as in the _grouped_f16 entries; other values ASVD_E_BADARG.
 *   Every other argument rule (token limits, alignment, leading dimensions, workspace) is that of the _f16 entry of the same name;
 *   asvd_lowrank_packed_work_bytes holds for both dtypes (2 bytes per element of z).  Deterministic, asynchronous. */
int asvd_w8_linear_a16(const void* x, int act_dtype, int64_t T, const void* q, int64_t ldq, const float* scale, const float* zero, int64_t group,
                       const void* bias, int64_t N, int64_t K, void* y, void* stream);
int asvd_wb_linear_a16(const void* x, int act_dtype, int64_t T, const void* q, int64_t ld_bytes, int bits, const float* scale, const float* zero,
                       int64_t group, const void* bias, int64_t N, int64_t K, void* y, void* stream);
int asvd_packed_gemm_a16(const void* x, int act_dtype, int64_t T, const void* q, int64_t ld_bytes, int bits, const float* scale, const float* zero,
                         int64_t group, const void* bias, int64_t N, int64_t K, void* y, void* stream);
int asvd_lowrank_packed_a16(const void* x, int act_dtype, int64_t T, const void* qB, int64_t ldB, const float* scaleB, const float* zeroB,
                            const void* qA, int64_t ldA, const float* scaleA, const float* zeroA, int bits, int64_t group, const void* bias,
                            int64_t N, int64_t K, int64_t r, void* y, void* work, size_t work_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * C1  collective for the one exchange step of the multi-GPU path: all-gather of the per-layer sensitivities over
 * RCCL (xGMI).  The reference has no distributed path; a maintainer who binds only this library gets the collective here, the
 * Python host side uses torch.distributed (same RCCL) for it.  RCCL is resolved at run time from the process (torch's
 * librccl when loaded, else librccl.so) — the library has no link-time dependency on it.
 *   asvd_comm_init     rank 0 creates the unique id and writes it to `id_path` (a file visible to all ranks of the node); the
 *                      other ranks wait for the file (up to timeout_s) and read it; all call ncclCommInitRank on `device`.
 *   asvd_comm_allgather_f32 / _f64   send [count] values, recv [count * nranks], device pointers, asynchronous on `stream`.
 *   asvd_comm_destroy  releases the communicator (rank 0 removes the id file).
 * Return ASVD_E_HIP when RCCL is missing or a call fails. */
int asvd_comm_init(void** comm_out, int rank, int nranks, int device, const char* id_path, int timeout_s);
int asvd_comm_allgather_f32(void* comm, const float* send, float* recv, int64_t count, void* stream);
int asvd_comm_allgather_f64(void* comm, const double* send, double* recv, int64_t count, void* stream);
int asvd_comm_destroy(void* comm);

/* ---------------------------------------------------------------------------------------------
 * Instrumentation: per-kernel-class wall time of the last asvd_svd_batched call, measured with HIP
 * events on the call's stream when enabled.  classes: 0 pack + Cholesky-QR reduction, 1 two-level Gram pass (sgram6),
 * 2 eigen-solves, 3 two-level update pass (supdate), 4 finalize, 5 snapshot (the blocked X^T X pass that opens a sparse sweep),
 * 6 single-level Gram, 7 single-level update, 8 fused two-level update + next-step Gram pass (supgram).
 * ms_host: float[9] total milliseconds; launches_host: int[9].  */
/* enabled: 0 off; 1 on, and a profiled call is never split (every kernel alone on the whole chip: what a rocprofv3 pass with ASVD_SPLIT=0 sees);
 * 2 on, and the call keeps the split of asvd_svd_set_split — both halves time their own launches on their own stream, asvd_svd_get_profile returns
 * the sums over both halves, asvd_svd_get_split_profile the halves one by one. */
void asvd_svd_set_profiling(int enabled);
int asvd_svd_get_profile(float* ms_host, int* launches_host);
/* The last call profiled in mode 2, by half: ms_host float[2*9], launches_host int[2*9] (half h, class c at [h*9 + c]); overlap_host float[4] =
 * {summed milliseconds inside the fused update + Gram launches (class 8) of half 0, of half 1, the UNION of those intervals on one time axis, the
 * time BOTH halves were inside such a launch}.  Returns 1 when that call ran split, 0 when it did not (the arrays are then stale). */
int asvd_svd_get_split_profile(float* ms_host, int* launches_host, float* overlap_host);
/* The split of a batch over the two halves of the chip, and what the library owns for it.
 * asvd_svd_batched runs a batch of >= 4 problems with >= 3072 columns as two halves, each on an internal stream masked to one half of the CUs
 * (hipExtStreamCreateWithCUMask): the eigen-solve launches of one half (VALU-bound) then overlap the HBM-bound update launches of the other,
 * which two launches of one stream never do.
 * OWNERSHIP — asvd_svd_batched (and asvd_svd, which calls it) is the only entry point of this header that creates anything behind the caller's
 * back.  Per CALLING HOST THREAD and device, at that
 * thread's first split call, the library creates (a) two CU-masked streams (hipExtStreamCreateWithCUMask has no flags argument: they are
 * ordinary blocking streams, i.e. they also order against the legacy NULL stream) and (b) ONE worker thread (it runs the second half; the
 * first half runs on the calling thread); both are released when the calling thread ends.  Per thread, so that two host threads making split
 * calls at once stay independent and the decision to split never depends on timing (results are those of the serial calls, bit for bit).
 * Per process and device, from the first asvd_svd_batched call of any size, (c) one file descriptor on /dev/shm/asvd_hip_split.<pci bus id>
 * holding a one-byte POSIX record lock: the presence of this process on the device.  No other call creates threads, streams or files;
 * workspaces and outputs are always the caller's.
 * REFUSALS — such a batch runs as ONE call on the caller's stream (ASVD_PATH_SPLIT_REFUSED) when another PROCESS that loaded this library
 * computes on the same device (the lock file: two ranks on one GPU would otherwise both claim "the first half + the second half") or when the
 * caller's stream is itself CU-masked (hipExtStreamGetCUMask).  A call profiled in mode 1 and a call under asvd_svd_set_call_cus are never split.
 *   asvd_svd_set_split(mode)   process-wide: 0 never split; 1 split when the rules above allow; -1 (default) as 1 unless ASVD_SPLIT=0 is set.
 *   asvd_svd_set_call_cus(cus) CUs the asvd_svd_batched calls of THIS host thread may use (0 = the whole device, the default): a caller that
 *                              drives calls on CU-masked streams of its own announces the count so that the launch geometry is sized for it. */
void asvd_svd_set_split(int mode);
void asvd_svd_set_call_cus(int cus);
/* Test hook: one launch of the two-level update kernel ([X_S X_T] <- [X_S X_T] Qfin for every super-pair of XOR step D) on
 * caller-built panels X [batch][nb][R][32]; Qfin [batch][npairs][128*128]; subact [batch][npairs][4] (pair updated when any flag is
 * set); done, nupd [batch] ints.  Used by tests/test_gpu_twolevel.py only. */
int asvd_test_supdate(float* X, int64_t panel_stride, int64_t batch_stride, int ns, int D, int R, int rows_per_wg,
                      const float* Qfin, const int* subact, const int* done, int* nupd, int nchunks, int npairs, int batch, void* stream);
/* Test hook: one launch of the fused kernel of the two-level sweep (update of XOR super-step D + partial Gram tiles of super-step E,
 * E != D) on caller-built panels.  Gx [batch][npairs][nchunks][6][32*32]: tiles [0,2] [0,3] [1,2] [1,3] [0,1] [2,3] of E's super-pairs
 * over the first m_pad rows, one partial per row chunk.  Din [batch][npairs][128]: squared norms of the 128 columns of every super-pair
 * of step D BEFORE the update, in the pair's column order (panels 2S, 2S+1, 2T, 2T+1; zeros for an absent member) — the power-of-two
 * column scales of the split-fp16 arithmetic come from them (in the library the eigen-solve launch of the step leaves them behind).
 * Other arguments as asvd_test_supdate.  tests/test_gpu_twolevel.py only. */
int asvd_test_supgram(float* X, int64_t panel_stride, int64_t batch_stride, int ns, int D, int E, int R, int m_pad, int rows_per_wg,
                      const float* Qfin, const int* subact, const float* Din, float* Gx, const int* done, int* nupd, int nchunks, int npairs,
                      int batch, void* stream);
/* Test hook: the Gram matrix G = X^T X of the Cholesky-QR reduction alone, on caller-built panels X [batch][nb][m_pad][32] (m_pad a multiple of
 * 32).  G [batch][32 nb][32 nb] doubles, upper 32-blocks written.  mode 0: fp64 matrix instructions (gram64_kernel); mode 1: the exact int8
 * digit path the library uses unless ASVD_GRAM_I8=0 (csrc/gram_i8.h): scratch >= 3 * 32 nb * 64 * batch bytes of device memory (digit planes:
 * the rows go in segments of what fits, at most seg_rows when seg_rows >= 64), ex = 32 nb ints per problem (column exponents, left behind).
 * tests/test_gpu_gram_i8.py only. */
int asvd_test_gram(const float* Xp, int64_t panel_stride, int64_t batch_stride, int nb, int m_pad, int batch, int mode, int seg_rows, double* G,
                   void* scratch, size_t scratch_bytes, int* ex, void* stream);
/* Test hook: the tile loop of the int8 digit-product kernels alone (csrc/i8_digits.h), with nw = 4 or 5 weights, over every 128 x 128 block of
 * two plane sets in that file's layout ([digit][panel][16-index group][column][16 bytes], strideA / strideB bytes per digit, npA / npB panels,
 * kgs 16-index groups: a multiple of 4, at most 2048).  out [nw][32 npA][32 npB] int32: out[s] = sum over a + c = s of (digit a of A)^T (digit c
 * of B).  tests/test_gpu_i8_stage_ring.py only. */
int asvd_test_i8_tile(const void* planesA, int64_t strideA, int npA, const void* planesB, int64_t strideB, int npB, int kgs, int nw, int* out,
                      void* stream);
/* Test hook: the super-panel pair schedule of the two-level sweeps for `ns` super-panels (grouped != 0: the grouped order where it applies,
 * else XOR).  out_dev: device int[out_capacity] >= nsteps * npairs; out[step * npairs + k] = (S << 16) | T or -1 (empty slot).
 * tests/test_gpu_twolevel.py only. */
int asvd_test_super_schedule(int ns, int grouped, int* out_dev, int out_capacity, int* nsteps_out, int* npairs_out);
/* Test hook: the wave-local 64x64 symmetric eigen-solver of the sweeps (csrc/evd_wave.h) alone, one wave per matrix, `sweeps` full
 * inner sweeps.  G [batch][64][64] symmetric; Q [batch][64][64] accumulated rotations (column = position, unsorted, unscaled);
 * diag / rnk / cs [batch][64]: eigenvalue estimate, descending-order rank and 1/|q_c| of every position; Gout: the image after the
 * sweeps; meas [batch][2]: the two off-diagonal measures of the input.  tests/test_gpu_evd_wave.py only. */
int asvd_test_evd_wave(const float* G, int batch, int sweeps, float* Q, float* diag, int* rnk, float* cs, float* Gout, float* meas, void* stream);
/* counts_host: long long[3] = {32-column panel-pair visits (one 64x64 eigen-solve each), pairs actually rotated, 128-column
 * super-pairs updated by the two-level sweeps (one 128-wide update pass over the rows each)} summed over the sweeps and problems of
 * the last profiled call: the algorithmic byte counts of the streaming kernels follow from these. */
int asvd_svd_get_pair_counts(long long* counts_host);
/* host wall time (ms) and rotated pairs of every Jacobi sweep of the last profiled call, whole batch together (the call
 * synchronises once per sweep).  Fills at most `cap` entries; returns the number of sweeps. */
int asvd_svd_get_sweep_times(float* ms_host, long long* rotated_host, int cap);

/* ---------------------------------------------------------------------------------------------
 * K20: one decode step of attention on a LOW-RANK KV cache (csrc/lowrank_kv.hip, DESIGN.md 4 "K20").
 * For a model whose k_proj / v_proj are SVDLinear(BLinear: hidden -> r, ALinear: r -> H_kv * D) the cache holds the BLinear outputs
 * ck [B, Tmax, r_k] and cv [B, Tmax, r_v] (fp16; row and batch strides in ELEMENTS, multiples of 8, 16-byte aligned bases) instead of K and V.
 * Ak [H_kv * D, r_k] and Av [H_kv * D, r_v] are the ALinear weights (fp16, contiguous), bk / bv their biases [H_kv * D] or NULL,
 * q [B, H, D] the query of the new token (already rotated in mode HALF), lens int32 [B] on the device with 0 <= lens[b] <= Tmax
 * (values outside are clamped), head h reads KV head h / (H / H_kv).  Replaces, for one new token, the reference's
 *     k = k_proj(x); v = v_proj(x); cat with the cached K, V; softmax(q k^T * scale) v        (K and V cached in full)
 * rope_mode ASVD_KV_ROPE_NONE: the scores use q~ = fp16(A_k^T q); bk adds one constant per head, drops out of the softmax and is ignored.
 * rope_mode ASVD_KV_ROPE_HALF: K is rebuilt tile by tile and rotated with rows of cos_tab / sin_tab (fp32 [Tmax, D/2], 16-byte aligned, row t
 *   for cache position t, pairs (i, i + D/2) as in HF rotate_half); bk must be NULL.
 * Served: dtype ASVD_F16 only, D 64 or 128, any H >= 1, H_kv dividing H, r_k and r_v multiples of 16 up to 16384, B >= 1.  Anything else,
 * a NULL or misaligned pointer or stride included, is ASVD_E_BADARG before any device call.  A sequence with lens[b] == 0 gets a zero row.
 * Nothing at cache positions >= lens[b] reaches an output; a non-finite value stays in its own sequence; results do not depend on timing.
 * All entries are asynchronous on `stream` (plain launches, graph-capturable); work is the caller's, 16-byte aligned.
 *   asvd_lowrank_kv_plan      host only: the token tile of the score kernels and the split length / count of the softmax-weighted sum for
 *                             (B, H, Tmax); the count is a function of these and of the 256 compute units of gfx950 parts alone.
 *   asvd_lowrank_kv_worksize  host only: bytes of `work` = q~ fp16 [B, Hpad, r_k] + scores fp32 [B, H, Tld] + (max, sum) and partial
 *                             sums fp32 [B, splits, Hpad, 2 + r_v], each rounded up to 256 bytes; Hpad = H up to 32, Tld = Tmax up to 16.
 *   asvd_lowrank_kv_scores    S[b, h, t] = scale * q_h . K_h[t] for t < lens[b] into the workspace and, if scores_out is not NULL,
 *                             to scores_out fp32 [B, H, Tmax] (zeros at t >= lens[b]).  Needs the first two parts of the workspace only.
 *   asvd_lowrank_kv_decode    all stages; out [B, H, D] fp16. */
#define ASVD_KV_ROPE_NONE 0
#define ASVD_KV_ROPE_HALF 1
int asvd_lowrank_kv_plan(int64_t B, int64_t H, int64_t Tmax, int64_t* token_tile, int64_t* split_len, int64_t* n_splits);
int asvd_lowrank_kv_worksize(int64_t B, int64_t H, int64_t Tmax, int64_t r_k, int64_t r_v, size_t* bytes);
int asvd_lowrank_kv_scores(const void* q, const void* ck, const void* lens, const void* Ak, const void* bk, const void* cos_tab, const void* sin_tab,
                           int dtype, int rope_mode, float scale, int64_t B, int64_t H, int64_t H_kv, int64_t D, int64_t r_k, int64_t Tmax,
                           int64_t ck_row_stride, int64_t ck_batch_stride, void* scores_out, void* work, size_t work_bytes, void* stream);
int asvd_lowrank_kv_decode(const void* q, const void* ck, const void* cv, const void* lens, const void* Ak, const void* Av, const void* bk,
                           const void* bv, const void* cos_tab, const void* sin_tab, int dtype, int rope_mode, float scale, int64_t B, int64_t H,
                           int64_t H_kv, int64_t D, int64_t r_k, int64_t r_v, int64_t Tmax, int64_t ck_row_stride, int64_t ck_batch_stride,
                           int64_t cv_row_stride, int64_t cv_batch_stride, void* out, void* work, size_t work_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K21: the low-rank KV cache as int8 codes (csrc/lowrank_kv_q8.hip, csrc/lowrank_kv_q8.h, DESIGN.md 4 "K21").
 * A cache row x[0 .. r) (r a multiple of 16) is cut into groups of 32 consecutive columns (a 16-wide last group when r % 32 == 16),
 * ng = ceil(r / 32) groups.  Per group amax = max |x|, s = amax / 127.0f (IEEE fp32), code = clamp(rintf(float(x) / s), -127, 127).
 * A group of zeros has s = 0 and codes 0; a group that holds a NaN or an Inf has s = NaN and codes 0.  The value a kernel uses is
 * d = fp16_rne(float(code) * s): one fp32 product, one rounding.
 * Layout: codes int8 [B, Tmax, r], unit column stride, row and batch strides (in BYTES) multiples of 16, 16-byte aligned base;
 * scales fp32 [B, Tmax, >= ng], unit last stride, row and batch strides in FLOATS, 4-byte aligned base.
 *   asvd_lowrank_kv_quant      x fp16 [B, n, r] (strides in elements, multiples of 8, 16-byte aligned base) -> codes and scales of the
 *                              B * n destination rows (the slice [:, t0 : t0 + n] of a cache: pass its first row and the cache's strides).
 *                              One launch, no host sync, no atomics; nothing outside those rows is written.
 *   asvd_lowrank_kv_scores_q8  asvd_lowrank_kv_scores / _decode with ck / cv holding codes and sk / sv their scales.  The kernels load codes
 *   asvd_lowrank_kv_decode_q8  and scales, dequantise in registers and feed the same products in the same order: the result has the bits of the
 *                              fp16 entry called on the dequantised cache.  Same workspace (asvd_lowrank_kv_worksize), same masking: nothing at
 *                              positions >= lens[b], code or scale, reaches an output.
 * dtype ASVD_F16 only.  A NULL or misaligned pointer, a rank that is no multiple of 16, a code stride that is no multiple of 16, a scale
 * row shorter than ng, a key bias under rotation and every rule of the fp16 entries are ASVD_E_BADARG before any device call. */
int asvd_lowrank_kv_quant(const void* x, int64_t x_row_stride, int64_t x_batch_stride, void* codes, int64_t c_row_stride, int64_t c_batch_stride,
                          void* scales, int64_t s_row_stride, int64_t s_batch_stride, int dtype, int64_t B, int64_t n, int64_t r, void* stream);
int asvd_lowrank_kv_scores_q8(const void* q, const void* ck, const void* sk, const void* lens, const void* Ak, const void* bk, const void* cos_tab,
                              const void* sin_tab, int dtype, int rope_mode, float scale, int64_t B, int64_t H, int64_t H_kv, int64_t D, int64_t r_k,
                              int64_t Tmax, int64_t ck_row_stride, int64_t ck_batch_stride, int64_t sk_row_stride, int64_t sk_batch_stride,
                              void* scores_out, void* work, size_t work_bytes, void* stream);
int asvd_lowrank_kv_decode_q8(const void* q, const void* ck, const void* cv, const void* sk, const void* sv, const void* lens, const void* Ak,
                              const void* Av, const void* bk, const void* bv, const void* cos_tab, const void* sin_tab, int dtype, int rope_mode,
                              float scale, int64_t B, int64_t H, int64_t H_kv, int64_t D, int64_t r_k, int64_t r_v, int64_t Tmax,
                              int64_t ck_row_stride, int64_t ck_batch_stride, int64_t cv_row_stride, int64_t cv_batch_stride, int64_t sk_row_stride,
                              int64_t sk_batch_stride, int64_t sv_row_stride, int64_t sv_batch_stride, void* out, void* work, size_t work_bytes,
                              void* stream);

/* ---------------------------------------------------------------------------------------------
 * K22: the four entries above for a bf16 model (csrc/lowrank_kv.hip, DESIGN.md 4 "K22").  Same argument lists, same rules, same workspace, same
 * error codes, every check before any device call; dtype is ASVD_F16 or ASVD_BF16 and names the type of q, Ak, Av, bk, bv, out and, for the
 * unquantised cache, of ck / cv.  With ASVD_F16 they ARE the entries above (which keep refusing every other dtype and forward here).  With ASVD_BF16:
 *   q~ = bf16(A_k^T q), p = bf16(exp(S - max)) (the sum l runs over the rounded p), out = bf16(acc / l + b_v): one round-to-nearest-even where
 *   the fp16 form rounds to fp16; every product is v_mfma_f32_32x32x16_bf16 with fp32 accumulation in the fp16 form's order; the rotation of mode
 *   HALF and the scores stay fp32; plan, workspace layout (q~ is two bytes either way), launch geometry and masking are unchanged.
 *   On an int8 cache the format does not change; a code's value is bf16_rne(fp16_rne(float(code) * s)), K21's value rounded once more
 *   (a double rounding by design: it is what dequantising to fp16 and converting to bf16 gives). */
int asvd_lowrank_kv_scores_a16(const void* q, const void* ck, const void* lens, const void* Ak, const void* bk, const void* cos_tab,
                               const void* sin_tab, int dtype, int rope_mode, float scale, int64_t B, int64_t H, int64_t H_kv, int64_t D, int64_t r_k,
                               int64_t Tmax, int64_t ck_row_stride, int64_t ck_batch_stride, void* scores_out, void* work, size_t work_bytes,
                               void* stream);
int asvd_lowrank_kv_decode_a16(const void* q, const void* ck, const void* cv, const void* lens, const void* Ak, const void* Av, const void* bk,
                               const void* bv, const void* cos_tab, const void* sin_tab, int dtype, int rope_mode, float scale, int64_t B, int64_t H,
                               int64_t H_kv, int64_t D, int64_t r_k, int64_t r_v, int64_t Tmax, int64_t ck_row_stride, int64_t ck_batch_stride,
                               int64_t cv_row_stride, int64_t cv_batch_stride, void* out, void* work, size_t work_bytes, void* stream);
int asvd_lowrank_kv_scores_q8_a16(const void* q, const void* ck, const void* sk, const void* lens, const void* Ak, const void* bk, const void* cos_tab,
                                  const void* sin_tab, int dtype, int rope_mode, float scale, int64_t B, int64_t H, int64_t H_kv, int64_t D,
                                  int64_t r_k, int64_t Tmax, int64_t ck_row_stride, int64_t ck_batch_stride, int64_t sk_row_stride,
                                  int64_t sk_batch_stride, void* scores_out, void* work, size_t work_bytes, void* stream);
int asvd_lowrank_kv_decode_q8_a16(const void* q, const void* ck, const void* cv, const void* sk, const void* sv, const void* lens, const void* Ak,
                                  const void* Av, const void* bk, const void* bv, const void* cos_tab, const void* sin_tab, int dtype, int rope_mode,
                                  float scale, int64_t B, int64_t H, int64_t H_kv, int64_t D, int64_t r_k, int64_t r_v, int64_t Tmax,
                                  int64_t ck_row_stride, int64_t ck_batch_stride, int64_t cv_row_stride, int64_t cv_batch_stride,
                                  int64_t sk_row_stride, int64_t sk_batch_stride, int64_t sv_row_stride, int64_t sv_batch_stride, void* out, void* work,
                                  size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ASVD_HIP_H */
