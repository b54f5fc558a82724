// w8_linear.hip — K12: forward and dequantization of RTN-quantized weights kept as uint8 codes (W8A16).
//
//   asvd_w8_linear_f16   y[T, N] = fp16( x[T, K] . w^T + bias ),   w[n, k] = fp16( scale[n] * (float(q[n, k]) - zero[n]) )
//   asvd_w8_dequant      out[n, k] = dtype( scale[n] * (float(q[n, k]) - zero[n]) )
//
// w is the value the fake quantizer of rtn_quant.hip writes: the subtraction (exact in fp32), ONE fp32 product, ONE rounding (RNE) to the
// weight dtype.  The forward dequantizes in registers to exactly that fp16 value and feeds it to the fp16 MFMA with fp32 accumulation, so
// the packed layer is nn.Linear on the fake-quantized weight up to the order of the fp32 sums.  The scale is NOT moved behind the
// accumulation (that would be a different model).
//
// Forward: a workgroup owns a (32-token tile, FT output features) tile of y, FT = 32, 16 or 8 (the 32-wide MFMA tile is partly filled
// with duplicate rows when few features per workgroup are needed to get a workgroup on every CU: the op is a weight stream).  Its four
// waves split the k iterations of 128 and reduce through LDS in a fixed order: no atomics, no barrier across workgroups, two calls give
// the same bits.  Operands go STRAIGHT from global memory to v_mfma_f32_32x32x16_f16 (the reduction index of an MFMA may be permuted as
// long as both operands use the same permutation, lowrank_forward.hip): lane (i, g) of a wave loads the 64 contiguous code bytes
// row i, k = 128 it + 64 g .. + 63 (four 16-byte loads; the two halves g of a row make a 128-byte segment) and the matching 128 bytes of
// x, and feeds 8-value chunk m of them to MFMA m of the iteration.  Rows beyond the tile's valid tokens / features re-read a valid row:
// an output element depends on its own two rows only, and those elements are not stored.  What K leaves beyond a multiple of 128 goes in
// 16-code chunks (16-byte loads while a chunk is whole, element loads for the last one, zero beyond K); rows that are not 16-byte aligned
// take element loads throughout.
//
// Non-finite activations: nothing multiplies a padding zero by an activation that exists (beyond K both operands are zero), so a token row
// with a NaN / +Inf / -Inf has the class of the fp64 evaluation of the same sums element for element, and every other row keeps its bits.
#include "common.h"
#include <atomic>

// every operation rounds on its own (the fake quantizer's `scale * (q - zero)` is a subtraction, then a product)
#pragma clang fp contract(off)

namespace {

constexpr int W8_THREADS = 256;
constexpr int W8_WAVES = W8_THREADS / 64;
constexpr int W8_KIT = 128;   // k values per iteration of a wave
constexpr int W8_MAX_DEVICES = 64;   // devices whose CU count the host entry caches
constexpr int W8_U = 2;       // iterations whose loads a wave issues before the first use

// the fp32 value scale * (code - zero).  It must exist as an fp32 value before the cast: the backend otherwise folds product + cast into one
// v_fma_mixlo_f16 (one rounding instead of the quantizer's two), whatever the contraction setting (rtn_quant.hip does the same)
__device__ __forceinline__ float w8_value(uint32_t word, int b, float scale, float zero) {
    float o = scale * ((float)((word >> (8 * b)) & 0xffu) - zero);
    asm volatile("" : "+v"(o));
    return o;
}

typedef float w8_f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 w8_f16x2 __attribute__((ext_vector_type(2)));

// four codes of one 32-bit word -> four fp16 values in two words (one packed conversion per pair); elements at or beyond `valid` (of this
// word) are zero
template <bool MASK>
__device__ __forceinline__ void w8_word_f16(uint32_t word, float scale, float zero, int valid, uint32_t& lo, uint32_t& hi) {
    w8_f32x2 a, b;
    a.x = w8_value(word, 0, scale, zero), a.y = w8_value(word, 1, scale, zero);
    b.x = w8_value(word, 2, scale, zero), b.y = w8_value(word, 3, scale, zero);
    lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(a, w8_f16x2));
    hi = __builtin_bit_cast(uint32_t, __builtin_convertvector(b, w8_f16x2));
    if (MASK) {
        lo &= (valid > 0 ? 0xffffu : 0u) | (valid > 1 ? 0xffff0000u : 0u);
        hi &= (valid > 2 ? 0xffffu : 0u) | (valid > 3 ? 0xffff0000u : 0u);
    }
}

// 16 codes -> the two 8-value MFMA operands
template <bool MASK>
__device__ __forceinline__ void w8_chunk_f16(const uint4& c, float scale, float zero, int valid, uint4& w0, uint4& w1) {
    w8_word_f16<MASK>(c.x, scale, zero, valid, w0.x, w0.y);
    w8_word_f16<MASK>(c.y, scale, zero, valid - 4, w0.z, w0.w);
    w8_word_f16<MASK>(c.z, scale, zero, valid - 8, w1.x, w1.y);
    w8_word_f16<MASK>(c.w, scale, zero, valid - 12, w1.z, w1.w);
}

// 16 code bytes at p[0..15], the first `valid` of them readable (zero for the others); constant indices only (no scratch)
__device__ __forceinline__ uint4 w8_load_codes_tail(const uint8_t* __restrict__ p, int valid) {
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 16; ++e)
        if (e < valid) w[e >> 2] |= (uint32_t)p[e] << (8 * (e & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// 8 fp16 values at p[0..7], the first `valid` of them readable
__device__ __forceinline__ uint4 w8_load_x_tail(const uint16_t* __restrict__ p, int valid) {
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if (e < valid) w[e >> 1] |= (uint32_t)p[e] << (16 * (e & 1));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ f32x16 w8_mfma(const uint4& a, const uint4& b, f32x16 acc) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
}

// one iteration of a lane: its 64 codes and 64 x values (16-byte loads), and the 8 MFMAs that consume them
__device__ __forceinline__ void w8_iter_load(uint4 (&cv)[4], uint4 (&xv)[8], const uint8_t* __restrict__ qrow, const uint16_t* __restrict__ xr, int it) {
    const uint4* cp = (const uint4*)(qrow + (int64_t)it * W8_KIT);
    const uint4* xp = (const uint4*)(xr + (int64_t)it * W8_KIT);
#pragma unroll
    for (int m = 0; m < 4; ++m) cv[m] = cp[m];
#pragma unroll
    for (int m = 0; m < 8; ++m) xv[m] = xp[m];
}

__device__ __forceinline__ f32x16 w8_iter_mfma(const uint4 (&cv)[4], const uint4 (&xv)[8], float sc, float zr, f32x16 acc) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        uint4 w0, w1;
        w8_chunk_f16<false>(cv[m], sc, zr, 16, w0, w1);
        acc = w8_mfma(xv[2 * m], w0, acc);
        acc = w8_mfma(xv[2 * m + 1], w1, acc);
    }
    return acc;
}

__global__ __launch_bounds__(W8_THREADS) void w8_linear_kernel(const uint16_t* __restrict__ x, int T, const uint8_t* __restrict__ q, int64_t ldq,
                                                              const float* __restrict__ scale, const float* __restrict__ zero,
                                                              const uint16_t* __restrict__ bias, int N, int K, uint16_t* __restrict__ y, int ft,
                                                              int nkfull /* whole iterations that take 16-byte loads */, int vec /* rows are 16-byte aligned */) {
    __shared__ float red[W8_WAVES][16 * 64];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int i = lane & 31, g = lane >> 5;
    const int n0 = blockIdx.x * ft, t0 = blockIdx.y * 32;
    const int nvalid = min(ft, N - n0), tvalid = min(32, T - t0);
    const int wrow = n0 + min(i, nvalid - 1), xrow = t0 + min(i, tvalid - 1);
    const float sc = scale[wrow], zr = zero[wrow];
    const uint8_t* qrow = q + (int64_t)wrow * ldq + 64 * g;
    const uint16_t* xr = x + (int64_t)xrow * K + 64 * g;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    // ---- whole iterations on aligned rows: 16-byte loads.  Groups of W8_U iterations have all their loads issued before the first use (with
    // one workgroup per CU a wave hides latency only by loads in flight); the iterations left over go one at a time ----
    int base = wave;
    for (; base + W8_WAVES * (W8_U - 1) < nkfull; base += W8_WAVES * W8_U) {
        uint4 cv[W8_U][4], xv[W8_U][8];
#pragma unroll
        for (int u = 0; u < W8_U; ++u) w8_iter_load(cv[u], xv[u], qrow, xr, base + W8_WAVES * u);
#pragma unroll
        for (int u = 0; u < W8_U; ++u) acc = w8_iter_mfma(cv[u], xv[u], sc, zr, acc);
    }
    for (; base < nkfull; base += W8_WAVES) {
        uint4 cv[4], xv[8];
        w8_iter_load(cv, xv, qrow, xr, base);
        acc = w8_iter_mfma(cv, xv, sc, zr, acc);
    }

    // ---- what is left (K % 128, or every iteration when the rows are not 16-byte aligned): chunk by chunk, zero beyond K ----
    const int nk = (K + W8_KIT - 1) / W8_KIT;
    // (iteration `it` belongs to wave it % 4 on both paths, so the result does not depend on which path the alignment selects)
    for (int it = nkfull + ((wave - nkfull) & (W8_WAVES - 1)); it < nk; it += W8_WAVES) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int k0 = it * W8_KIT + 64 * g + 16 * m;       // first k of this lane's chunk
            const int valid = max(0, min(16, K - k0));
            const uint8_t* cp = qrow + (int64_t)it * W8_KIT + 16 * m;
            const uint16_t* xp = xr + (int64_t)it * W8_KIT + 16 * m;
            uint4 c, x0, x1;
            if (vec && valid == 16) {   // a whole chunk of aligned rows (K % 128 >= 16): 16-byte loads here too
                c = *(const uint4*)cp;
                x0 = ((const uint4*)xp)[0];
                x1 = ((const uint4*)xp)[1];
            } else {
                c = w8_load_codes_tail(cp, valid);
                x0 = w8_load_x_tail(xp, min(8, valid));
                x1 = w8_load_x_tail(xp + 8, valid - 8);
            }
            uint4 w0, w1;
            w8_chunk_f16<true>(c, sc, zr, valid, w0, w1);
            acc = w8_mfma(x0, w0, acc);
            acc = w8_mfma(x1, w1, acc);
        }
    }

    // ---- the four partial tiles, summed in a fixed order ----
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][r * 64 + lane] = acc[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int e = tid + W8_THREADS * r, reg = e >> 6, l = e & 63;
        const int row = (reg & 3) + 8 * (reg >> 2) + 4 * (l >> 5), col = l & 31;   // token, feature of accumulator register `reg` of lane `l`
        if (col < nvalid && row < tvalid) {
            float v = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
            if (bias) v += f16_bits_to_f32(bias[n0 + col]);
            y[(int64_t)(t0 + row) * N + n0 + col] = f32_to_f16_bits(v);
        }
    }
}

// ---- dequantization to a dense weight ---------------------------------------------------------------------------------------------
// one thread per 16 consecutive codes of a row, 16-byte loads and stores (cols % 16 == 0, aligned rows)
template <int DT>
__global__ __launch_bounds__(W8_THREADS) void w8_dequant_kernel(const uint8_t* __restrict__ q, int64_t ldq, const float* __restrict__ scale,
                                                               const float* __restrict__ zero, int64_t rows, int64_t cols, void* __restrict__ out,
                                                               int64_t ldo) {
    const int64_t chunks = (cols + 15) / 16;
    const int64_t id = (int64_t)blockIdx.x * W8_THREADS + threadIdx.x;
    if (id >= rows * chunks) return;
    const int64_t row = id / chunks, c0 = (id - row * chunks) * 16;
    const float sc = scale[row], zr = zero[row];
    const uint8_t* qp = q + row * ldq + c0;
    typename elem<DT>::T* op = (typename elem<DT>::T*)out + row * ldo + c0;
    {
        const uint4 c = *(const uint4*)qp;
        const uint32_t w[4] = {c.x, c.y, c.z, c.w};
        if (DT == ASVD_F32) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                ((uint4*)op)[j] = make_uint4(__float_as_uint(w8_value(w[j], 0, sc, zr)), __float_as_uint(w8_value(w[j], 1, sc, zr)),
                                             __float_as_uint(w8_value(w[j], 2, sc, zr)), __float_as_uint(w8_value(w[j], 3, sc, zr)));
        } else {
            uint32_t h[8];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const float a = w8_value(w[j], 2 * p, sc, zr), b = w8_value(w[j], 2 * p + 1, sc, zr);
                    h[2 * j + p] = DT == ASVD_F16 ? ((uint32_t)f32_to_f16_bits(a) | ((uint32_t)f32_to_f16_bits(b) << 16))
                                                  : ((uint32_t)f32_to_bf16_bits(a) | ((uint32_t)f32_to_bf16_bits(b) << 16));
                }
            ((uint4*)op)[0] = make_uint4(h[0], h[1], h[2], h[3]);
            ((uint4*)op)[1] = make_uint4(h[4], h[5], h[6], h[7]);
        }
    }
}

// rows that do not allow 16-byte accesses (odd ranks): one element per thread, consecutive lanes on consecutive columns
template <int DT>
__global__ __launch_bounds__(W8_THREADS) void w8_dequant_elem_kernel(const uint8_t* __restrict__ q, int64_t ldq, const float* __restrict__ scale,
                                                                    const float* __restrict__ zero, int64_t rows, int64_t cols,
                                                                    void* __restrict__ out, int64_t ldo) {
    const int64_t id = (int64_t)blockIdx.x * W8_THREADS + threadIdx.x;
    if (id >= rows * cols) return;
    const int64_t row = id / cols, c = id - row * cols;
    elem<DT>::st(out, row * ldo + c, w8_value((uint32_t)q[row * ldq + c], 0, scale[row], zero[row]));
}

}  // namespace

extern "C" {

int64_t asvd_w8_linear_max_tokens(void) { return ASVD_W8_MAX_TOKENS; }

int asvd_w8_linear_f16(const void* x, int64_t T, const void* q, int64_t ldq, const float* scale, const float* zero, const void* bias, int64_t N,
                       int64_t K, void* y, void* stream) {
    if (!x || !q || !scale || !zero || !y) return ASVD_E_BADARG;
    if (T < 1 || T > ASVD_W8_MAX_TOKENS || N < 1 || K < 1 || ldq < K || N > 0x7fffffff - 64 || K > 0x7fffffff - 256) return ASVD_E_BADARG;
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)bias) & 1) return ASVD_E_BADARG;   // fp16 elements
    // per-call host cost matters at decode size: the CU count of the first W8_MAX_DEVICES devices is looked up once (relaxed atomics: two
    // threads may both look it up and store the same value); devices beyond that are asked every call
    static std::atomic<int> s_cus[W8_MAX_DEVICES];
    int dev = 0;
    ASVD_HIP_CHECK(hipGetDevice(&dev));
    int cus = (dev >= 0 && dev < W8_MAX_DEVICES) ? s_cus[dev].load(std::memory_order_relaxed) : 0;
    if (!cus) {
        ASVD_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        if (cus < 1) return ASVD_E_HIP;
        if (dev >= 0 && dev < W8_MAX_DEVICES) s_cus[dev].store(cus, std::memory_order_relaxed);
    }
    const int nT = (int)((T + 31) / 32);
    // the widest feature tile that still puts a workgroup on every CU (bandwidth-bound: more streams win over fuller MFMA tiles)
    int ft = 32;
    while (ft > 8 && nT * ceil_div64(N, ft) < cus) ft /= 2;
    const bool vec = ((uintptr_t)x % 16 == 0) && ((uintptr_t)q % 16 == 0) && (K % 8 == 0) && (ldq % 16 == 0);
    const int nkfull = vec ? (int)(K / W8_KIT) : 0;
    hipLaunchKernelGGL(w8_linear_kernel, dim3((unsigned)ceil_div64(N, ft), (unsigned)nT), dim3(W8_THREADS), 0, (hipStream_t)stream,
                       (const uint16_t*)x, (int)T, (const uint8_t*)q, ldq, scale, zero, (const uint16_t*)bias, (int)N, (int)K, (uint16_t*)y, ft,
                       nkfull, vec ? 1 : 0);
    ASVD_HIP_CHECK(hipGetLastError());
    return ASVD_OK;
}

int asvd_w8_dequant(const void* q, int64_t ldq, const float* scale, const float* zero, int64_t rows, int64_t cols, void* out, int out_dtype,
                    int64_t ldo, void* stream) {
    if (!q || !scale || !zero || !out || rows < 1 || cols < 1 || ldq < cols || ldo < cols || !dtype_ok(out_dtype)) return ASVD_E_BADARG;
    const int64_t es = (int64_t)dtype_size(out_dtype);
    if ((uintptr_t)out % es) return ASVD_E_BADARG;
    const bool vec_ok = (cols % 16 == 0) && ((uintptr_t)q % 16 == 0) && (ldq % 16 == 0) && ((uintptr_t)out % 16 == 0) && ((ldo * es) % 16 == 0);
    const int64_t grid = ceil_div64(vec_ok ? rows * (cols / 16) : rows * cols, W8_THREADS);
    if (grid > 0x7fffffff) return ASVD_E_BADARG;
    if (vec_ok) {
        ASVD_DISPATCH_DTYPE(out_dtype, DT,
                            hipLaunchKernelGGL(w8_dequant_kernel<DT>, dim3((unsigned)grid), dim3(W8_THREADS), 0, (hipStream_t)stream, (const uint8_t*)q,
                                               ldq, scale, zero, rows, cols, out, ldo));
    } else {
        ASVD_DISPATCH_DTYPE(out_dtype, DT,
                            hipLaunchKernelGGL(w8_dequant_elem_kernel<DT>, dim3((unsigned)grid), dim3(W8_THREADS), 0, (hipStream_t)stream,
                                               (const uint8_t*)q, ldq, scale, zero, rows, cols, out, ldo));
    }
    ASVD_HIP_CHECK(hipGetLastError());
    return ASVD_OK;
}

}  // extern "C"
