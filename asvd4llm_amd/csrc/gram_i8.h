// gram_i8.h — the fp64 Gram matrix of the Cholesky-QR reduction computed EXACTLY on the int8 matrix pipe (included by svd_jacobi.hip inside
// its anonymous namespace, after tall_kernels.h and i8_digits.h, which holds the exponent rules, the digit packer and the tile loop).  Round 6.
//
// gram64_kernel runs at what v_mfma_f64_16x16x4 delivers (49.7 TFLOP/s: 45 ms per 32 x 4096^2, the largest single item of the reduction).
// The Cholesky-QR needs G to ~1e-16 cond^2, which rules out every rounded product — but not an EXACT Gram matrix of a matrix that differs
// from X by a column-wise tiny perturbation (that is a backward error of the same kind as, and smaller than, the fp32 rounding of R that
// follows).  So (Ozaki-style error-free splitting, specialised to a Gram product):
//   1. every column j gets a power of two 2^E_j just above its largest magnitude (colmaxexp_kernel; max |x| 2^-E_j < 127/128);
//   2. t = rint(x 2^(23 - E_j)) is a 24-bit signed integer, written as three balanced radix-256 digits t = d0 2^16 + d1 2^8 + d2 with
//      d0 in [-127, 127], d1, d2 in [-128, 127] (split_i8_kernel: three int8 planes in MFMA operand order) — entries within a factor 2 of the
//      column's largest are kept exactly, the others to 2^-24 of it: |x~ - x| <= 2^(E_j - 24), about 2e-7 of the column norm for a
//      Gaussian-like column (fp32 itself: 6e-8);
//   3. gram_i8_kernel accumulates the nine digit products D_a^T D_b with v_mfma_i32_32x32x32_i8 into FIVE int32 accumulators, one per
//      weight s = a + b (at most 3 x 2^14 per row and accumulator: exact in int32 for <= 32768 rows; longer problems go in row segments that
//      are added in fp64), and combines them as sum_s P_s 2^(8 (4 - s)) 2^(E_i + E_j - 46) in fp64: the exact Gram matrix of X~ up to the
//      2^-53 of that last sum.
// 9 x 2 x 4096^3 / 2 integer operations per 4096^2 problem at ~2 Pop/s instead of 6.9e10 fp64 flop at 49.7 TFLOP/s.
// Inf / NaN in a column: its exponent is a sentinel and its row and column of G come out NaN, as gram64_kernel's do.
#pragma once

// ex[b][col] = E with  max_r |X[r][col]| 2^-E < 127/128;  dn[b][col] (optional) = |x_col|_2 in fp64, fixed summation order
// (grid: (nb, batch), 256 threads: lane = column, eight row lanes)
__global__ __launch_bounds__(256) void colmaxexp_kernel(const float* __restrict__ X, int64_t panel_stride, int64_t batch_stride, int m_pad,
                                                        int n_pad, int* __restrict__ ex, double* __restrict__ dn) {
    __shared__ unsigned smax[8][PB];
    __shared__ double ssq[8][PB];
    const int P = blockIdx.x, b = blockIdx.y, c = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const float* __restrict__ xp = X + (int64_t)b * batch_stride + (int64_t)P * panel_stride + c;
    unsigned mx = 0;
    double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
    for (int r = rl; r < m_pad; r += 32) {  // m_pad is a multiple of 32: four independent loads per trip
        const float x0 = xp[(int64_t)r * PB], x1 = xp[(int64_t)(r + 8) * PB], x2 = xp[(int64_t)(r + 16) * PB], x3 = xp[(int64_t)(r + 24) * PB];
        const unsigned a0 = __float_as_uint(x0) & 0x7fffffffu, a1 = __float_as_uint(x1) & 0x7fffffffu;
        const unsigned a2 = __float_as_uint(x2) & 0x7fffffffu, a3 = __float_as_uint(x3) & 0x7fffffffu;
        const unsigned m01 = a0 > a1 ? a0 : a1, m23 = a2 > a3 ? a2 : a3, m4 = m01 > m23 ? m01 : m23;
        mx = mx > m4 ? mx : m4;
        q0 = fma((double)x0, (double)x0, q0); q1 = fma((double)x1, (double)x1, q1);
        q2 = fma((double)x2, (double)x2, q2); q3 = fma((double)x3, (double)x3, q3);
    }
    smax[rl][c] = mx;
    ssq[rl][c] = (q0 + q1) + (q2 + q3);
    __syncthreads();
    if (rl == 0) {
        double q = ssq[0][c];
#pragma unroll
        for (int i = 1; i < 8; ++i) { mx = mx > smax[i][c] ? mx : smax[i][c]; q += ssq[i][c]; }
        ex[(int64_t)b * n_pad + P * PB + c] = gi_exp_of_bits(mx);
        if (dn) dn[(int64_t)b * n_pad + P * PB + c] = sqrt(q);
    }
}

// exs[b][i] = ex[b][perm[b][i]], dp[b][i] = d[b][perm[b][i]]: exponents and norms in sorted-column order; inv[b][perm[b][i]] = i
__global__ void perm_gather_kernel(const int* __restrict__ ex, const double* __restrict__ d, const int* __restrict__ perm, int n, int* __restrict__ exs,
                                   double* __restrict__ dp, int* __restrict__ inv) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = blockIdx.y;
    const int q = perm[(int64_t)b * n + i];
    exs[(int64_t)b * n + i] = ex[(int64_t)b * n + q];
    dp[(int64_t)b * n + i] = d[(int64_t)b * n + q];
    inv[(int64_t)b * n + q] = i;
}

// Digit planes of the rows [r0, r0 + 16 kgs) of every problem:  planes[b][digit a][panel P][16-row group kg][column c][16 bytes = rows], the
// operand order of gi_tile_loop (i8_digits.h).  Rows >= m_pad are zero.
// grid: (nb, ceil(kgs / 8), batch), 256 threads = 8 row groups x 32 columns.  The workgroup READS panel P of X (coalesced) and writes column q = 32 P + c
// to plane position inv[q] (nullable: q itself) — a scatter of 16-byte pieces.  (First version: plane panel P GATHERED its columns perm[32 P + c], every lane
// of a load in another panel's 128-byte row: 5.6 ms per 32 x 4096^2 against 0.7 ms unpermuted.)
__global__ __launch_bounds__(256) void split_i8_kernel(const float* __restrict__ X, int64_t panel_stride, int64_t batch_stride, int nb, int m_pad,
                                                       int n_pad, const int* __restrict__ ex /* exponents of the columns of X, in X's order */, int r0, int kgs,
                                                       signed char* __restrict__ planes, int64_t plane_stride /* bytes per digit and problem = nb kgs 512 */,
                                                       const int* __restrict__ inv /* nullable: plane position of every column of X */,
                                                       const int* __restrict__ done /* nullable: problems whose flag is set are skipped */) {
    const int P = blockIdx.x, b = blockIdx.z, c = threadIdx.x & 31;
    const int kg = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (kg >= kgs || (done && ld_flag(done + b))) return;
    const int q = P * PB + c;
    const int E = ex[(int64_t)b * n_pad + q];
    const int pos = inv ? inv[(int64_t)b * n_pad + q] : q;
    const float* __restrict__ xp = X + (int64_t)b * batch_stride + (int64_t)P * panel_stride + c;
    unsigned w0[4] = {0, 0, 0, 0}, w1[4] = {0, 0, 0, 0}, w2[4] = {0, 0, 0, 0};
    if (E != GI_BAD && E != GI_ZERO) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = r0 + kg * 16 + i;
            const float x = r < m_pad ? xp[(int64_t)r * PB] : 0.0f;
            gi_pack_digits((int)rintf(ldexpf(x, 23 - E)), i, w0, w1, w2);  // exact scaling, |t| <= 127 * 2^16
        }
    }
    gi_store_digits(planes + (int64_t)b * 3 * plane_stride + ((int64_t)(pos >> 5) * kgs + kg) * 512 + (pos & 31) * 16, plane_stride, w0, w1, w2);
}

// G[b] (upper 32-blocks, I <= J) (+)= exact Gram matrix of the digitised rows of this segment.
// grid (upper-triangular 128 x 128 blocks, batch), 512 threads: gi_tile_loop with all five weights, the plane set on both sides.
__global__ __launch_bounds__(512) void gram_i8_kernel(const signed char* __restrict__ planes, int64_t plane_stride, int nb, int kgs, int n_pad,
                                                      const int* __restrict__ ex, double* __restrict__ G, int64_t ldg, int64_t g_batch_stride,
                                                      int accumulate, int nt, const double* __restrict__ dp /* nullable: G_ij / (dp_i dp_j) is stored;
                                                      a column with dp = 0 gets a unit diagonal and zeros */) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gi_lds[];  // GI_LDS_BYTES
    int Ib, Jb;
    gi_tri_block(nt, Ib, Jb);
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wi = w >> 2, wj = w & 3;
    const signed char* __restrict__ pl = planes + (int64_t)b * 3 * plane_stride;
    i32x16 acc[2][5];
    gi_tile_loop<5>(pl, plane_stride, nb, pl, plane_stride, nb, Ib, Jb, kgs, gi_lds, acc);
    const int J = 4 * Jb + wj;
    if (J >= nb) return;
    const int j = lane & 31;
    double sj = gi_scale(ex[(int64_t)b * n_pad + J * PB + j]);
    if (dp) { const double dj = dp[(int64_t)b * n_pad + J * PB + j]; sj = dj > 0.0 ? sj / dj : (dj == 0.0 ? 0.0 : __builtin_nan("")); }
    double* __restrict__ out = G + (int64_t)b * g_batch_stride;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int I = 4 * Ib + 2 * wi + t;
        if (I > J || I >= nb) continue;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int i = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
            double si = gi_scale(ex[(int64_t)b * n_pad + I * PB + i]);
            bool unit = false;
            if (dp) {
                const double di = dp[(int64_t)b * n_pad + I * PB + i];
                si = di > 0.0 ? si / di : (di == 0.0 ? 0.0 : __builtin_nan(""));
                unit = di == 0.0 && I == J && i == j;
            }
            double v = (double)acc[t][4][reg];
            v += (double)acc[t][3][reg] * 256.0;
            v += (double)acc[t][2][reg] * 65536.0;
            v += (double)acc[t][1][reg] * 16777216.0;
            v += (double)acc[t][0][reg] * 4294967296.0;
            v = v * si * sj;
            const int64_t o = (int64_t)(I * PB + i) * ldg + J * PB + j;
            v = accumulate ? out[o] + v : v;
            out[o] = unit ? 1.0 : v;
        }
    }
}
