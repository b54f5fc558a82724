// snapshot_i8.h — the coupling snapshot of the sparse sweeps (fullcheck_kernel, jacobi_kernels.h) on the int8 matrix pipe (included by
// svd_jacobi.hip inside its anonymous namespace, after i8_digits.h and gram_i8.h).  Round 6.
//
// The snapshot is X^T X of the working matrix, read only through |g_ij| / sqrt(g_ii g_jj) against tol = 1e-6 (which pairs still rotate) and through
// its maximum (the termination measure).  fullcheck_kernel forms it from three fp16 products per fp32 product, splitting the operands inside the
// GEMM loop: 12.4 ms per 32 x 4096^2, bound by the L2 -> LDS operand traffic.  Here the columns are digitised once (split_i8_kernel of gram_i8.h:
// 24-bit fixed point under a power of two just above the column's LARGEST entry, measured in the pass that sums the squares) and the eight digit
// products of weight <= 3 are accumulated exactly in four int32 accumulators by gi_tile_loop of i8_digits.h (eight waves, 64 x 32 per wave); only
// the product of the two lowest digits is dropped, 2^-32 of the largest product.  A cosine comes out to <= ~1e-7 of the worst case (entries
// rounded to 2^-25 of the column maximum), against the 1e-6 it is compared with.
// (Measured first and WRONG: six products, weight <= 2, with exponents from the column norms — entries of a dense 4096-row column sit seven bits
// below their norm, their value lives in the two LOW digits, and the dropped weight-3 products were the second largest terms: a noise floor of
// ~5e-5 on the cosines marked nearly every pair, sparse sweeps of 129 / 107 / 92 ms instead of 37 / 24 / 17.)
// Problems of more than 32768 rows keep fullcheck_kernel (int32 range).
#pragma once

// panel_sumsq_kernel (jacobi_kernels.h) + the exponent of the column maximum in the same pass: dn[b][col] = sum of squares (fp32, same order as
// panel_sumsq_kernel), ex[b][col] = E with max |x| 2^-E < 127/128.  grid (nb, batch), 256 threads.
__global__ __launch_bounds__(256) void panel_sumsq_max_kernel(const float* __restrict__ X, int64_t panel_stride, int64_t batch_stride, int m_pad, int n_pad,
                                                              float* __restrict__ dn, int* __restrict__ ex, const int* __restrict__ done) {
    const int I = blockIdx.x, b = blockIdx.y, c = threadIdx.x & 31, g = threadIdx.x >> 5;
    if (ld_flag(done + b)) return;
    const float* __restrict__ P = X + (int64_t)b * batch_stride + (int64_t)I * panel_stride;
    float s = 0.0f;
    unsigned mx = 0;
    for (int r = g; r < m_pad; r += 8) {
        const float x = P[(int64_t)r * PB + c];
        s = fmaf(x, x, s);
        const unsigned a = __float_as_uint(x) & 0x7fffffffu;
        mx = mx > a ? mx : a;
    }
    __shared__ float red[8][32];
    __shared__ unsigned rmx[8][32];
    red[g][c] = s;
    rmx[g][c] = mx;
    __syncthreads();
    if (g == 0) {
        float t = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i) { t += red[i][c]; mx = mx > rmx[i][c] ? mx : rmx[i][c]; }
        dn[(int64_t)b * n_pad + I * PB + c] = t;
        ex[(int64_t)b * n_pad + I * PB + c] = gi_exp_of_bits(mx);
    }
}

// grid (upper-triangular 128 x 128 blocks, batch), 512 threads; the plane set on both sides of gi_tile_loop, then the mark step of fullcheck_kernel.
__global__ __launch_bounds__(512) void fullcheck_i8_kernel(const signed char* __restrict__ planes, int64_t plane_stride, int nb, int kgs, int n_pad,
                                                           const int* __restrict__ ex, const float* __restrict__ dn, float tol, int kb,
                                                           unsigned char* __restrict__ pflag, unsigned* __restrict__ maxoff_bits,
                                                           const int* __restrict__ done, int nt) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gi_lds[];  // GI_LDS_BYTES
    const int b = blockIdx.y;
    if (ld_flag(done + b)) return;
    int Ib, Jb;
    gi_tri_block(nt, Ib, Jb);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wi = w >> 2, wj = w & 3;
    const signed char* __restrict__ pl = planes + (int64_t)b * 3 * plane_stride;
    i32x16 acc[2][4];
    gi_tile_loop<4>(pl, plane_stride, nb, pl, plane_stride, nb, Ib, Jb, kgs, gi_lds, acc);
    const int J = 4 * Jb + wj;
    if (J >= nb) return;
    const float* __restrict__ dnb = dn + (int64_t)b * n_pad;
    const int* __restrict__ exb = ex + (int64_t)b * n_pad;
    const float dj = dnb[J * PB + (lane & 31)];
    const int Ej = exb[J * PB + (lane & 31)];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int I = 4 * Ib + 2 * wi + t;
        if (I > J || I >= nb) continue;
        snapshot_mark(I, J, lane, dnb, dj, tol, kb, nb, b, pflag, maxoff_bits, [&](int reg, int i, float) {
            const int Ei = exb[I * PB + i];
            // sum of the kept digit products, in units of 2^8: |.| < 2^55, exact in fp64 up to its last bit; the power-of-two scales bring it back to the data
            const double sum = (double)acc[t][3][reg] + (double)acc[t][2][reg] * 256.0 + (double)acc[t][1][reg] * 65536.0 + (double)acc[t][0][reg] * 16777216.0;
            float g = 0.0f;
            if (Ei == GI_BAD || Ej == GI_BAD) g = __builtin_nanf("");
            else if (Ei != GI_ZERO && Ej != GI_ZERO) g = (float)ldexp(sum, Ei + Ej - 38);
            return g;
        });
    }
}
