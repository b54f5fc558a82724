// reorth.hip — K18: make the columns of Q [m, k] orthonormal in their given order (asvd_reorth_batched, include/asvd_hip.h).
//
// One pass:  E = Q^T Q - I,  T = striu(E) + diag(E) / 2,  Q <- Q - Q T : the first-order inverse of the Cholesky factor of Q^T Q.  Every pass
// multiplies Q from the right by an upper-triangular matrix with a positive diagonal, so the leading j columns keep their span for every j and the
// limit is the Cholesky-QR factor of the input.  The host repeats passes until max |E| <= tol (one read of the per-problem maxima per pass).
//
//   reorth_colexp_kernel   power-of-two exponent of every column (i8_digits.h rules)
//   reorth_split_kernel    24-bit fixed-point columns as three int8 digit planes in gi_tile_loop's operand order, straight from row-major Q
//   reorth_e_kernel        E on the upper 32-blocks: the EXACT Gram matrix of the digitised columns (nine digit products on the int8 matrix pipe,
//                          gi_tile_loop<5>), combined in fp64, identity subtracted in fp64, then rounded to fp32 and stored as T; max |E| per problem
//   reorth_update_kernel   Q <- Q - Q T in place with the fp32 matrix instructions: a workgroup owns 128 rows and walks the column tiles in
//                          DESCENDING order (output column j depends on input columns <= j only)
// Nothing here sums in an order that depends on timing: the integer products are exact, the fp64 combination and the fp32 update have one fixed
// order, and max |E| is an integer maximum over bit patterns of magnitudes (order-independent by construction; NaN patterns rank above all numbers).
#include "common.h"
#include <algorithm>
#include <cstring>
#include <vector>

namespace {

#include "i8_digits.h"

constexpr int RO_PB = 32;             // columns per panel (gi_tile_loop)
constexpr int RO_SEG_ROWS = 32768;    // rows per exact int32 accumulation (i8_digits.h: 3 x 2^14 per row and accumulator)
constexpr int RU_ROWS = 128, RU_COLS = 128;  // update kernel: rows per workgroup (32 per wave), columns per tile
constexpr float RO_REFUSE = 0.25f;    // entry max |E| above which a problem is refused

// ex[b][col] = E with max_r |Q[r][col]| 2^-E < 127/128 (GI_ZERO: zero or padding column, GI_BAD: Inf / NaN).  grid (nb, batch), 256 threads
__global__ __launch_bounds__(256) void reorth_colexp_kernel(const float* const* __restrict__ Qs, int m, int k, int64_t ldq, int kp, int* __restrict__ ex,
                                                            const int* __restrict__ active) {
    __shared__ unsigned smax[8][RO_PB];
    const int b = blockIdx.y;
    if (!ld_flag(active + b)) return;
    const int c = threadIdx.x & 31, rl = threadIdx.x >> 5, col = blockIdx.x * RO_PB + c;
    const float* __restrict__ q = Qs[b];
    unsigned mx = 0;
    if (col < k)
        for (int r = rl; r < m; r += 8) {
            const unsigned a = __float_as_uint(q[(int64_t)r * ldq + col]) & 0x7fffffffu;
            mx = mx > a ? mx : a;
        }
    smax[rl][c] = mx;
    __syncthreads();
    if (rl == 0) {
#pragma unroll
        for (int i = 1; i < 8; ++i) mx = mx > smax[i][c] ? mx : smax[i][c];
        ex[(int64_t)b * kp + col] = gi_exp_of_bits(mx);
    }
}

// digit planes of rows [r0, r0 + 16 kgs) : planes[b][digit][panel][kg][column][16 bytes = rows]; rows >= m and columns >= k are zero.
// grid (nb, ceil(kgs / 8), batch), 256 threads = 8 row groups x 32 columns
__global__ __launch_bounds__(256) void reorth_split_kernel(const float* const* __restrict__ Qs, int m, int k, int64_t ldq, int kp, const int* __restrict__ ex,
                                                           int r0, int kgs, signed char* __restrict__ planes, int64_t plane_stride,
                                                           const int* __restrict__ active) {
    const int P = blockIdx.x, b = blockIdx.z, c = threadIdx.x & 31;
    const int kg = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (kg >= kgs || !ld_flag(active + b)) return;
    const int col = P * RO_PB + c;
    const int E = ex[(int64_t)b * kp + col];
    const float* __restrict__ q = Qs[b];
    unsigned w0[4] = {0, 0, 0, 0}, w1[4] = {0, 0, 0, 0}, w2[4] = {0, 0, 0, 0};
    if (col < k && E != GI_BAD && E != GI_ZERO) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = r0 + kg * 16 + i;
            const float x = r < m ? q[(int64_t)r * ldq + col] : 0.0f;
            gi_pack_digits((int)rintf(ldexpf(x, 23 - E)), i, w0, w1, w2);
        }
    }
    gi_store_digits(planes + (int64_t)b * 3 * plane_stride + ((int64_t)P * kgs + kg) * 512 + c * 16, plane_stride, w0, w1, w2);
}

// T[b] (upper 32-blocks) from the digit planes of one row segment.  first: the segment's Gram block minus the identity is stored; otherwise it is
// added to what is stored.  last: max |E| over the k x k part goes to maxbits[b], and the block is rewritten as T = striu(E) + diag(E) / 2 (zero
// below the diagonal and beyond k).  One segment (m <= 32768): E is rounded to fp32 once, after the identity is subtracted in fp64.
// grid (upper-triangular 128 x 128 blocks, batch), 512 threads
__global__ __launch_bounds__(512) void reorth_e_kernel(const signed char* __restrict__ planes, int64_t plane_stride, int nb, int kgs, int kp, int k,
                                                       const int* __restrict__ ex, float* __restrict__ T, int64_t ldt, int64_t t_stride, int first,
                                                       int last, int nt, unsigned* __restrict__ maxbits, const int* __restrict__ active) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gi_lds[];  // GI_LDS_BYTES
    const int b = blockIdx.y;
    if (!ld_flag(active + b)) return;
    int Ib, Jb;
    gi_tri_block(nt, Ib, Jb);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wi = w >> 2, wj = w & 3;
    const signed char* __restrict__ pl = planes + (int64_t)b * 3 * plane_stride;
    i32x16 acc[2][5];
    gi_tile_loop<5>(pl, plane_stride, nb, pl, plane_stride, nb, Ib, Jb, kgs, gi_lds, acc);
    const int J = 4 * Jb + wj;
    if (J >= nb) return;
    const int j = lane & 31, gj = J * RO_PB + j;
    const double sj = gi_scale(ex[(int64_t)b * kp + gj]);
    float* __restrict__ out = T + (int64_t)b * t_stride;
    unsigned mx = 0;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int I = 4 * Ib + 2 * wi + t;
        if (I > J || I >= nb) continue;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int i = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), gi = I * RO_PB + i;
            const double si = gi_scale(ex[(int64_t)b * kp + gi]);
            double v = (double)acc[t][4][reg];
            v += (double)acc[t][3][reg] * 256.0;
            v += (double)acc[t][2][reg] * 65536.0;
            v += (double)acc[t][1][reg] * 16777216.0;
            v += (double)acc[t][0][reg] * 4294967296.0;
            v = v * si * sj;
            const int64_t o = (int64_t)gi * ldt + gj;
            float e;
            if (first) e = (float)(gi == gj ? v - 1.0 : v);
            else e = out[o] + (float)v;
            if (last) {
                const bool inside = gi < k && gj < k;
                if (inside) {
                    const unsigned a = __float_as_uint(e) & 0x7fffffffu;
                    mx = mx > a ? mx : a;
                }
                e = (!inside || gi > gj) ? 0.0f : (gi == gj ? 0.5f * e : e);
            }
            out[o] = e;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned other = (unsigned)__shfl_xor((int)mx, o, 64);
        mx = mx > other ? mx : other;
    }
    if (lane == 0 && mx) atomicMax(maxbits + b, mx);
}

// Q[b] <- Q[b] - Q[b] T[b], in place.  grid (ceil(m / 128), batch), 256 threads: wave w owns rows 32 w .. 32 w + 31 of the workgroup's 128 and
// reads and writes no other row.  Column tiles of 128 in descending order; tile jt sums over the 32-column blocks I <= 4 jt + 3 of Q (T is zero below
// its diagonal, so the tile's own blocks add nothing to the columns left of them): everything tile jt reads lies at or left of it and is still input.
// Per block I: T[32 x 128] and the wave's Q[32 x 32] go through LDS (the A operand wants lane = row), the next block's loads are in flight in
// registers behind the 64 matrix instructions of this one.  (Tiles of 64 columns re-read Q twice as often: 42 ms per update of 32 x 4096^2.)
__global__ __launch_bounds__(256) void reorth_update_kernel(float* const* __restrict__ Qs, int m, int k, int64_t ldq, int nb, const float* __restrict__ T,
                                                            int64_t ldt, int64_t t_stride, const int* __restrict__ active) {
    __shared__ float sT[32][160];     // row stride 160 = 32 mod 64: the two half-waves of a B read (rows kk, kk + 1) fall on disjoint banks
    __shared__ float sA[4][32][33];
    const int b = blockIdx.y;
    if (!ld_flag(active + b)) return;
    float* __restrict__ q = Qs[b];
    const float* __restrict__ tb = T + (int64_t)b * t_stride;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int row0 = blockIdx.x * RU_ROWS + 32 * w;
    const int l31 = lane & 31, lh = lane >> 5;
    for (int jt = (k + RU_COLS - 1) / RU_COLS - 1; jt >= 0; --jt) {
        f32x16 acc0, acc1, acc2, acc3;
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc0[i] = 0.0f; acc1[i] = 0.0f; acc2[i] = 0.0f; acc3[i] = 0.0f; }
        const int nI = min(4 * jt + 4, nb);
        float rt[16], ra[16];
        auto fetch = [&](int I) {
#pragma unroll
            for (int i = 0; i < 16; ++i) rt[i] = tb[(int64_t)(I * 32 + (tid >> 7) + 2 * i) * ldt + jt * RU_COLS + (tid & 127)];  // inside [kp, ldt]: ldt = 128 ceil(k / 128)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = row0 + lh + 2 * i, col = I * 32 + l31;
                ra[i] = (row < m && col < k) ? q[(int64_t)row * ldq + col] : 0.0f;
            }
        };
        fetch(0);
        for (int I = 0; I < nI; ++I) {
            __syncthreads();  // every wave is done reading the block before
#pragma unroll
            for (int i = 0; i < 16; ++i) sT[(tid >> 7) + 2 * i][tid & 127] = rt[i];
#pragma unroll
            for (int i = 0; i < 16; ++i) sA[w][lh + 2 * i][l31] = ra[i];
            __syncthreads();
            if (I + 1 < nI) fetch(I + 1);
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const float a = sA[w][l31][2 * s + lh];
                const float b0 = sT[2 * s + lh][l31], b1 = sT[2 * s + lh][32 + l31], b2 = sT[2 * s + lh][64 + l31], b3 = sT[2 * s + lh][96 + l31];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc1, 0, 0, 0);
                acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b2, acc2, 0, 0, 0);
                acc3 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b3, acc3, 0, 0, 0);
            }
        }
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int row = row0 + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
            if (row >= m) continue;
            const int c0 = jt * RU_COLS + l31, c1 = c0 + 32, c2 = c0 + 64, c3 = c0 + 96;
            float* __restrict__ qr = q + (int64_t)row * ldq;
            if (c0 < k) qr[c0] = qr[c0] - acc0[reg];
            if (c1 < k) qr[c1] = qr[c1] - acc1[reg];
            if (c2 < k) qr[c2] = qr[c2] - acc2[reg];
            if (c3 < k) qr[c3] = qr[c3] - acc3[reg];
        }
    }
}

struct ReorthLayout {
    int nb, nt, kp, kgs_max;
    int64_t ldt, plane_stride_max;
    size_t per_problem, fixed;
    int sub;
};

// workspace of one sub-batch: pointer table, exponents, maxima, activity flags, digit planes of one row segment, T
ReorthLayout reorth_layout(int batch, int64_t m, int64_t k) {
    ReorthLayout L;
    L.nb = (int)ceil_div64(k, RO_PB);
    L.nt = (L.nb + 3) / 4;
    L.kp = L.nb * RO_PB;
    L.ldt = round_up64(k, RU_COLS);
    L.kgs_max = (int)round_up64(ceil_div64(std::min<int64_t>(m, RO_SEG_ROWS), 16), 4);
    L.plane_stride_max = (int64_t)L.nb * L.kgs_max * 512;
    L.per_problem = (size_t)3 * L.plane_stride_max + (size_t)L.ldt * L.ldt * sizeof(float) + (size_t)L.kp * sizeof(int) + 64;
    L.fixed = 4096;
    const size_t cap = (size_t)1 << 30;  // sub-batches of at most 1 GiB (one problem when a single one is larger)
    L.sub = (int)std::max<size_t>(1, std::min<size_t>((size_t)batch, cap / L.per_problem));
    return L;
}

}  // namespace

extern "C" {

int asvd_reorth_worksize(int batch, int64_t m, int64_t k, size_t* bytes) {
    if (!bytes || batch < 1 || k < 1 || m < k || m > 0x7fffffff) return ASVD_E_BADARG;
    const ReorthLayout L = reorth_layout(batch, m, k);
    *bytes = L.fixed + (size_t)L.sub * L.per_problem + (size_t)L.sub * 64;
    return ASVD_OK;
}

int asvd_reorth_batched(int batch, float* const* Q_host, int64_t m, int64_t k, int64_t ldq, int max_passes, float tol, void* work, size_t work_bytes,
                        int* info_host, void* stream) {
    if (batch < 1 || !Q_host || !work || k < 1 || m < k || ldq < k || m > 0x7fffffff) return ASVD_E_BADARG;
    for (int b = 0; b < batch; ++b)
        if (!Q_host[b] || ((uintptr_t)Q_host[b] % sizeof(float)) != 0) return ASVD_E_BADARG;
    size_t need = 0;
    if (asvd_reorth_worksize(batch, m, k, &need) != ASVD_OK) return ASVD_E_BADARG;
    if (work_bytes < need) return ASVD_E_WORKSPACE;
    if (max_passes <= 0) max_passes = 8;
    if (!(tol > 0.0f)) tol = 2e-6f;
    hipStream_t st = (hipStream_t)stream;
    const ReorthLayout L = reorth_layout(batch, m, k);
    const int nseg = (int)ceil_div64(m, RO_SEG_ROWS);
    ASVD_HIP_CHECK(hipFuncSetAttribute((const void*)reorth_e_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, GI_LDS_BYTES));

    int worst = ASVD_OK;
    for (int b0 = 0; b0 < batch; b0 += L.sub) {
        const int nbt = std::min(L.sub, batch - b0);
        char* p = (char*)work;
        auto take = [&](size_t bytes) { char* q = p; p += (bytes + 15) & ~(size_t)15; return (void*)q; };
        float** q_dev = (float**)take((size_t)nbt * sizeof(void*));
        unsigned* maxbits = (unsigned*)take((size_t)nbt * sizeof(unsigned));
        int* active = (int*)take((size_t)nbt * sizeof(int));
        int* ex = (int*)take((size_t)nbt * L.kp * sizeof(int));
        signed char* planes = (signed char*)take((size_t)nbt * 3 * L.plane_stride_max);
        float* T = (float*)take((size_t)nbt * L.ldt * L.ldt * sizeof(float));
        const int64_t t_stride = L.ldt * L.ldt;
        ASVD_HIP_CHECK(hipMemcpyAsync(q_dev, Q_host + b0, (size_t)nbt * sizeof(void*), hipMemcpyHostToDevice, st));
        ASVD_HIP_CHECK(hipMemsetAsync(T, 0, (size_t)nbt * t_stride * sizeof(float), st));  // the blocks below the diagonal are never written

        std::vector<int> act(nbt, 1), status(nbt, ASVD_OK), passes(nbt, 0);
        std::vector<unsigned> bits(nbt, 0), e_in(nbt, 0), e_out(nbt, 0);
        auto as_float = [](unsigned u) { float f; memcpy(&f, &u, sizeof f); return f; };

        // E (as T) and max |E| of every active problem; one stream synchronisation
        auto measure = [&]() -> int {
            ASVD_HIP_CHECK(hipMemcpyAsync(active, act.data(), (size_t)nbt * sizeof(int), hipMemcpyHostToDevice, st));
            ASVD_HIP_CHECK(hipMemsetAsync(maxbits, 0, (size_t)nbt * sizeof(unsigned), st));
            reorth_colexp_kernel<<<dim3(L.nb, nbt), 256, 0, st>>>(q_dev, (int)m, (int)k, ldq, L.kp, ex, active);
            for (int s = 0; s < nseg; ++s) {
                const int r0 = s * RO_SEG_ROWS;
                const int kgs = (int)round_up64(ceil_div64(std::min<int64_t>(m - r0, RO_SEG_ROWS), 16), 4);
                const int64_t plane_stride = (int64_t)L.nb * kgs * 512;
                reorth_split_kernel<<<dim3(L.nb, (kgs + 7) / 8, nbt), 256, 0, st>>>(q_dev, (int)m, (int)k, ldq, L.kp, ex, r0, kgs, planes, plane_stride, active);
                reorth_e_kernel<<<dim3(L.nt * (L.nt + 1) / 2, nbt), 512, GI_LDS_BYTES, st>>>(planes, plane_stride, L.nb, kgs, L.kp, (int)k, ex, T, L.ldt, t_stride,
                                                                                            s == 0, s == nseg - 1, L.nt, maxbits, active);
            }
            ASVD_HIP_CHECK(hipGetLastError());
            ASVD_HIP_CHECK(hipMemcpyAsync(bits.data(), maxbits, (size_t)nbt * sizeof(unsigned), hipMemcpyDeviceToHost, st));
            ASVD_HIP_CHECK(hipStreamSynchronize(st));
            return ASVD_OK;
        };

        int rc = measure();
        if (rc != ASVD_OK) return rc;
        int nact = 0;
        for (int b = 0; b < nbt; ++b) {
            e_in[b] = e_out[b] = bits[b];
            const float e = as_float(bits[b]);
            if (bits[b] >= 0x7f800000u) { status[b] = ASVD_N_NAN; act[b] = 0; }
            else if (e > RO_REFUSE) { status[b] = ASVD_N_NOCONV; act[b] = 0; }
            else if (e <= tol) act[b] = 0;
            nact += act[b];
        }
        for (int pass = 1; nact > 0; ++pass) {
            ASVD_HIP_CHECK(hipMemcpyAsync(active, act.data(), (size_t)nbt * sizeof(int), hipMemcpyHostToDevice, st));
            reorth_update_kernel<<<dim3((unsigned)ceil_div64(m, RU_ROWS), nbt), 256, 0, st>>>(q_dev, (int)m, (int)k, ldq, L.nb, T, L.ldt, t_stride, active);
            rc = measure();
            if (rc != ASVD_OK) return rc;
            nact = 0;
            for (int b = 0; b < nbt; ++b) {
                if (!act[b]) continue;
                passes[b] = pass;
                e_out[b] = bits[b];
                const float e = as_float(bits[b]);
                if (bits[b] >= 0x7f800000u || e >= 1.0f) { status[b] = ASVD_N_NOCONV; act[b] = 0; }
                else if (e <= tol) act[b] = 0;
                else if (pass >= max_passes) { status[b] = ASVD_N_NOCONV; act[b] = 0; }
                nact += act[b];
            }
        }
        for (int b = 0; b < nbt; ++b) {
            if (info_host) {
                int* o = info_host + 4 * (int64_t)(b0 + b);
                o[0] = status[b]; o[1] = passes[b]; o[2] = (int)e_in[b]; o[3] = (int)e_out[b];
            }
            worst = std::max(worst, status[b]);
        }
    }
    return worst;
}

}  // extern "C"
