// w8_linear.hip — K12: forward and dequantization of RTN-quantized weights kept as uint8 codes (W8A16).
//
//   asvd_w8_linear_f16   y[T, N] = fp16( x[T, K] . w^T + bias ),   w[n, k] = fp16( scale[n] * (float(q[n, k]) - zero[n]) )
//   asvd_w8_linear_a16   the same with the activation dtype (fp16 / bf16: K19 below) and the group size as arguments; the _f16 entries forward to it
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
// K13, codes stored at their own width (bits = 6 or 4): a row is a little-endian bitstream, code k in bits [bits k, bits (k + 1)) of the row read
// as one integer, zero-padded to whole blocks of 64 codes (8 bits bytes: 48 or 32).  Block 2 it + g is exactly what lane (i, g) owns in iteration
// `it`, so the tile loop is the one above with three or two 16-byte loads per lane and iteration instead of four; the codes are cut out of the
// loaded words with constant shifts (w8_code) and go through the same subtraction, product and conversion, chunk m to MFMA m, so
// asvd_wb_linear_f16 gives the bits of asvd_w8_linear_f16 on the same codes.  asvd_wb_pack / asvd_wb_dequant write and read the format.
//
// K14, group-wise scales (GROUPED): scale / zero are [N, ng] with one pair per G = 64 or 128 codes of a row, ng = ceil(K / G).  The 64 codes a lane
// owns in an iteration (k = 128 it + 64 g .. + 63) lie in ONE group, (128 it + 64 g) >> log2 G, so the lane loads one scale and one zero per
// iteration, next to its code loads, and everything else is the loop above: the same tiles, the same k split, the same order of every sum.
//
// K17, inputs beyond decode (asvd_packed_gemm_f16): the same weight and the same operands on a token-tiled GEMM that stages x through LDS once per
// workgroup and dequantizes a lane's codes once per up to 128 tokens; its description stands with packed_gemm_kernel below.
//
// K19, bf16 activations (the asvd_*_a16 entries with act_dtype ASVD_BF16): every forward kernel here takes the activation type ADT as its first
// template parameter.  The bf16 form has w = bf16(scale * (code - zero)) (the same fp32 value behind the same barrier, ONE packed RNE conversion:
// the bits w8_dequant_kernel<ASVD_BF16> writes for finite values), v_mfma_f32_32x32x16_bf16 on the same operands (the operand and accumulator
// layout of the fp16 instruction), a bf16 bias and an RNE-rounded bf16 output (K16: a bf16 z, and a bf16 NaN as poison); everything else is
// the one text, and the fp16 instantiations are what they were before the parameter existed.
//
// Non-finite activations: nothing multiplies a padding zero by an activation that exists (beyond K both operands are zero), so a token row
// with a NaN / +Inf / -Inf has the class of the fp64 evaluation of the same sums element for element, and every other row keeps its bits.
#include "common.h"
#include "grid_sync.h"
#include <atomic>

// every operation rounds on its own (the fake quantizer's `scale * (q - zero)` is a subtraction, then a product)
#pragma clang fp contract(off)

namespace {

constexpr int W8_THREADS = 256;
constexpr int W8_WAVES = W8_THREADS / 64;
constexpr int W8_KIT = 128;   // k values per iteration of a wave
constexpr int W8_MAX_DEVICES = 64;   // devices whose CU count the host entry caches
constexpr int W8_U = 2;       // iterations whose loads a wave issues before the first use
constexpr int W8_ROW_SHIFT = 62;   // the "group shift" of per-row scales in the dequantization kernels

// 32-bit words that hold a chunk of 16 codes of BITS bits, and with it 16-byte words that hold a lane's block of 64
template <int BITS> constexpr int W8_CW = BITS / 2;

// code j (a constant after unrolling) of the 16 codes in w[]: bits [BITS j, BITS (j + 1)) of the words read as one little-endian integer.  At 8
// and 4 bits no code crosses a word; at 6 bits codes 5 and 10 do
template <int BITS>
__device__ __forceinline__ uint32_t w8_code(const uint32_t (&w)[W8_CW<BITS>], int j) {
    const int bit = BITS * j, lo = bit >> 5, sh = bit & 31;
    uint32_t v = w[lo] >> sh;
    if (sh + BITS > 32) v |= w[lo + 1 < W8_CW<BITS> ? lo + 1 : lo] << ((32 - sh) & 31);
    return v & ((1u << BITS) - 1u);
}

// the fp32 value scale * (code - zero).  It must exist as an fp32 value before the cast: the backend otherwise folds product + cast into one
// v_fma_mixlo_f16 (one rounding instead of the quantizer's two), whatever the contraction setting (rtn_quant.hip does the same)
__device__ __forceinline__ float w8_value(uint32_t code, float scale, float zero) {
    float o = scale * ((float)code - zero);
    asm volatile("" : "+v"(o));
    return o;
}

typedef float w8_f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 w8_f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 w8_bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 w8_bf16x8 __attribute__((ext_vector_type(8)));

// ADT, the activation type of the forward kernels (ASVD_F16 or ASVD_BF16): the type of x, bias, y and of the weight operand the codes are
// dequantized to.  The two forms differ in the four helpers below (pair conversion, element load, element store, matrix instruction) and in
// the NaN K16 poisons with; tiles, k permutation, split of k over the waves and the order of every sum are one text.
// two fp32 values -> one packed pair, ONE rounding (RNE) each (bf16: v_cvt_pk_bf16_f32).  For finite values the bf16 bits are those of
// f32_to_bf16_bits (common.h), which is what w8_dequant_kernel<ASVD_BF16> writes
template <int ADT>
__device__ __forceinline__ uint32_t w8_cvt_pair(w8_f32x2 v) {
    if constexpr (ADT == ASVD_BF16) return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, w8_bf16x2));
    else return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, w8_f16x2));
}
template <int ADT>
__device__ __forceinline__ float w8_act_to_f32(uint16_t b) {
    return ADT == ASVD_BF16 ? bf16_bits_to_f32(b) : f16_bits_to_f32(b);
}
template <int ADT>
__device__ __forceinline__ uint16_t w8_f32_to_act(float v) {
    if constexpr (ADT == ASVD_BF16) return __builtin_bit_cast(uint16_t, (__bf16)v);   // RNE
    else return f32_to_f16_bits(v);
}
template <int ADT> constexpr uint16_t W8_ACT_NAN = ADT == ASVD_BF16 ? 0x7fc0 : 0x7e00;   // 0x7e00 is a FINITE bf16 number

// 16 codes -> the two 8-value MFMA operands (one packed conversion per pair of codes); elements at or beyond `valid` are zero
template <int ADT, int BITS, bool MASK>
__device__ __forceinline__ void w8_chunk_f16(const uint32_t (&w)[W8_CW<BITS>], float scale, float zero, int valid, uint4& w0, uint4& w1) {
    uint32_t h[8];
#pragma unroll
    for (int p = 0; p < 8; p += 2) {   // four values, then their two conversions
        w8_f32x2 a, b;
        a.x = w8_value(w8_code<BITS>(w, 2 * p), scale, zero), a.y = w8_value(w8_code<BITS>(w, 2 * p + 1), scale, zero);
        b.x = w8_value(w8_code<BITS>(w, 2 * p + 2), scale, zero), b.y = w8_value(w8_code<BITS>(w, 2 * p + 3), scale, zero);
        h[p] = w8_cvt_pair<ADT>(a);
        h[p + 1] = w8_cvt_pair<ADT>(b);
        if (MASK) {
            h[p] &= (valid > 2 * p ? 0xffffu : 0u) | (valid > 2 * p + 1 ? 0xffff0000u : 0u);
            h[p + 1] &= (valid > 2 * p + 2 ? 0xffffu : 0u) | (valid > 2 * p + 3 ? 0xffff0000u : 0u);
        }
    }
    w0 = make_uint4(h[0], h[1], h[2], h[3]);
    w1 = make_uint4(h[4], h[5], h[6], h[7]);
}

// word c (a constant after unrolling) of a 16-byte load
__device__ __forceinline__ uint32_t w8_word(const uint4& v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }

// the words of chunk m (16 codes) of a lane's 64-code block, loaded as BITS / 2 16-byte words
template <int BITS>
__device__ __forceinline__ void w8_chunk_words(const uint4 (&cv)[W8_CW<BITS>], int m, uint32_t (&w)[W8_CW<BITS>]) {
#pragma unroll
    for (int t = 0; t < W8_CW<BITS>; ++t) w[t] = w8_word(cv[(W8_CW<BITS> * m + t) >> 2], (W8_CW<BITS> * m + t) & 3);
}

// 16 code bytes at p[0..15], the first `valid` of them readable (zero for the others); constant indices only (no scratch)
__device__ __forceinline__ uint4 w8_load_codes_tail(const uint8_t* __restrict__ p, int valid) {
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 16; ++e)
        if (e < valid) w[e >> 2] |= (uint32_t)p[e] << (8 * (e & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// 8 fp16 / bf16 values at p[0..7], the first `valid` of them readable
__device__ __forceinline__ uint4 w8_load_x_tail(const uint16_t* __restrict__ p, int valid) {
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if (e < valid) w[e >> 1] |= (uint32_t)p[e] << (16 * (e & 1));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

template <int ADT>
__device__ __forceinline__ f32x16 w8_mfma(const uint4& a, const uint4& b, f32x16 acc) {
    if constexpr (ADT == ASVD_BF16)
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(w8_bf16x8, a), __builtin_bit_cast(w8_bf16x8, b), acc, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
}

// one iteration of a lane: its 64 codes (8 BITS bytes) and 64 x values (16-byte loads), and the 8 MFMAs that consume them
template <int BITS, bool XCOH>
__device__ __forceinline__ void w8_iter_load(uint4 (&cv)[W8_CW<BITS>], uint4 (&xv)[8], const uint8_t* __restrict__ qrow, const uint16_t* __restrict__ xr,
                                             int it) {
    const uint4* cp = (const uint4*)(qrow + (int64_t)it * (W8_KIT * BITS / 8));
    const uint4* xp = (const uint4*)(xr + (int64_t)it * W8_KIT);
#pragma unroll
    for (int m = 0; m < W8_CW<BITS>; ++m) cv[m] = cp[m];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        if constexpr (XCOH) xv[m] = z_load16(xp + m);   // the intermediate of the packed pair (K16), written in this launch: agent-scope loads
        else xv[m] = xp[m];
    }
}

template <int ADT, int BITS>
__device__ __forceinline__ f32x16 w8_iter_mfma(const uint4 (&cv)[W8_CW<BITS>], const uint4 (&xv)[8], float sc, float zr, f32x16 acc) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        uint32_t w[W8_CW<BITS>];
        uint4 w0, w1;
        w8_chunk_words<BITS>(cv, m, w);
        w8_chunk_f16<ADT, BITS, false>(w, sc, zr, 16, w0, w1);
        acc = w8_mfma<ADT>(xv[2 * m], w0, acc);
        acc = w8_mfma<ADT>(xv[2 * m + 1], w1, acc);
    }
    return acc;
}

// One (32-token, ft-feature) tile of y = ADT(x w^T + bias), tokens t0.., features n0.., by the whole workgroup: the tile loop, the LDS
// reduction in its fixed order, bias and store.  w8_linear_kernel is one call of it; the packed pair calls it once per unit of a phase (the
// caller separates two calls by a __syncthreads(): red is reused).
// BITS = 8: q holds one code per byte, ldq >= K.  BITS = 6, 4: q holds the bitstream rows (ldq bytes apart), K % 16 == 0 and everything is
// 16-byte aligned (vec is 1).  GROUPED: scale / zero are [N, ng], a group is 1 << gshift codes; K % 16 == 0 and vec is 1 at every width.
// XCOH: x is the pair's intermediate (z_load16; vec is 1 and K % 16 == 0, no element loads of x).  ZOUT: y is that intermediate (z_store).
template <int ADT, int BITS, bool GROUPED, bool XCOH, bool ZOUT>
__device__ __forceinline__ void w8_tile(float (&red)[W8_WAVES][16 * 64], const uint16_t* __restrict__ x, int T, const uint8_t* __restrict__ q, int64_t ldq,
                                        const float* __restrict__ scale, const float* __restrict__ zero, const uint16_t* __restrict__ bias, int N,
                                        int K, uint16_t* __restrict__ y, int t0, int n0, int ft,
                                        int nkfull /* whole iterations that take 16-byte loads */, int vec /* rows are 16-byte aligned */, int ng,
                                        int gshift) {
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int i = lane & 31, g = lane >> 5;
    const int nvalid = min(ft, N - n0), tvalid = min(32, T - t0);
    const int wrow = n0 + min(i, nvalid - 1), xrow = t0 + min(i, tvalid - 1);
    float sc = 0.f, zr = 0.f;
    if constexpr (!GROUPED) sc = scale[wrow], zr = zero[wrow];
    // GROUPED: the row's scales and zeros; the lane's block of iteration `it` lies in group (W8_KIT it + 64 g) >> gshift
    const float* srow = scale + (GROUPED ? (int64_t)wrow * ng : 0);
    const float* zrow = zero + (GROUPED ? (int64_t)wrow * ng : 0);
    const uint8_t* qrow = q + (int64_t)wrow * ldq + 8 * BITS * g;   // the lane's 64-code block of iteration 0
    const uint16_t* xr = x + (int64_t)xrow * K + 64 * g;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    // ---- whole iterations on aligned rows: 16-byte loads.  Groups of W8_U iterations have all their loads issued before the first use (with
    // one workgroup per CU a wave hides latency only by loads in flight); the iterations left over go one at a time ----
    int base = wave;
    for (; base + W8_WAVES * (W8_U - 1) < nkfull; base += W8_WAVES * W8_U) {
        uint4 cv[W8_U][W8_CW<BITS>], xv[W8_U][8];
        float gs[W8_U], gz[W8_U];   // GROUPED: in flight with the code loads of the group (a whole iteration lies within K: the index is < ng)
#pragma unroll
        for (int u = 0; u < W8_U; ++u) {
            w8_iter_load<BITS, XCOH>(cv[u], xv[u], qrow, xr, base + W8_WAVES * u);
            if constexpr (GROUPED) {
                const int gi = ((base + W8_WAVES * u) * W8_KIT + 64 * g) >> gshift;
                gs[u] = srow[gi], gz[u] = zrow[gi];
            }
        }
#pragma unroll
        for (int u = 0; u < W8_U; ++u) acc = w8_iter_mfma<ADT, BITS>(cv[u], xv[u], GROUPED ? gs[u] : sc, GROUPED ? gz[u] : zr, acc);
    }
    for (; base < nkfull; base += W8_WAVES) {
        uint4 cv[W8_CW<BITS>], xv[8];
        w8_iter_load<BITS, XCOH>(cv, xv, qrow, xr, base);
        if constexpr (GROUPED) {
            const int gi = (base * W8_KIT + 64 * g) >> gshift;
            sc = srow[gi], zr = zrow[gi];
        }
        acc = w8_iter_mfma<ADT, BITS>(cv, xv, sc, zr, acc);
    }

    // ---- what is left (K % 128, or every iteration when the rows are not 16-byte aligned): chunk by chunk, zero beyond K ----
    const int nk = (K + W8_KIT - 1) / W8_KIT;
    // (iteration `it` belongs to wave it % 4 on both paths, so the result does not depend on which path the alignment selects)
    for (int it = nkfull + ((wave - nkfull) & (W8_WAVES - 1)); it < nk; it += W8_WAVES) {
        uint4 cv[W8_CW<BITS>];
        if constexpr (GROUPED) {
            // the lane's four chunks lie in one group (G % 64 == 0).  A block that starts at or beyond K has no group: it reads the row's last
            // pair, and its chunks are masked below
            const int gi = min((it * W8_KIT + 64 * g) >> gshift, ng - 1);
            sc = srow[gi], zr = zrow[gi];
        }
        if (BITS != 8) {   // the lane's block as a whole (rows are padded to whole blocks); a block that starts at or beyond K is not there
#pragma unroll
            for (int m = 0; m < W8_CW<BITS>; ++m)
                cv[m] = it * W8_KIT + 64 * g < K ? ((const uint4*)(qrow + (int64_t)it * (W8_KIT * BITS / 8)))[m] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int k0 = it * W8_KIT + 64 * g + 16 * m;       // first k of this lane's chunk
            const int valid = max(0, min(16, K - k0));
            const uint16_t* xp = xr + (int64_t)it * W8_KIT + 16 * m;
            uint32_t w[W8_CW<BITS>];
            uint4 x0, x1;
            if (BITS != 8) {   // K % 16 == 0: a chunk is whole or absent; the padding codes of an absent one are masked below, x is zero
                w8_chunk_words<BITS>(cv, m, w);
                if constexpr (XCOH) {
                    x0 = valid == 16 ? z_load16((const uint4*)xp) : make_uint4(0, 0, 0, 0);
                    x1 = valid == 16 ? z_load16((const uint4*)xp + 1) : make_uint4(0, 0, 0, 0);
                } else {
                    x0 = valid == 16 ? ((const uint4*)xp)[0] : make_uint4(0, 0, 0, 0);
                    x1 = valid == 16 ? ((const uint4*)xp)[1] : make_uint4(0, 0, 0, 0);
                }
            } else {
                const uint8_t* cp = qrow + (int64_t)it * W8_KIT + 16 * m;
                uint4 c;
                if constexpr (XCOH) {   // aligned rows and K % 16 == 0: a chunk is whole or absent
                    c = valid == 16 ? *(const uint4*)cp : make_uint4(0, 0, 0, 0);
                    x0 = valid == 16 ? z_load16((const uint4*)xp) : make_uint4(0, 0, 0, 0);
                    x1 = valid == 16 ? z_load16((const uint4*)xp + 1) : make_uint4(0, 0, 0, 0);
                } else if (vec && valid == 16) {   // a whole chunk of aligned rows (K % 128 >= 16): 16-byte loads here too
                    c = *(const uint4*)cp;
                    x0 = ((const uint4*)xp)[0];
                    x1 = ((const uint4*)xp)[1];
                } else {
                    c = w8_load_codes_tail(cp, valid);
                    x0 = w8_load_x_tail(xp, min(8, valid));
                    x1 = w8_load_x_tail(xp + 8, valid - 8);
                }
#pragma unroll
                for (int t = 0; t < W8_CW<BITS>; ++t) w[t] = w8_word(c, t & 3);
            }
            uint4 w0, w1;
            w8_chunk_f16<ADT, BITS, true>(w, sc, zr, valid, w0, w1);
            acc = w8_mfma<ADT>(x0, w0, acc);
            acc = w8_mfma<ADT>(x1, w1, acc);
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
            if (bias) v += w8_act_to_f32<ADT>(bias[n0 + col]);
            if constexpr (ZOUT) z_store(y + (int64_t)(t0 + row) * N + n0 + col, w8_f32_to_act<ADT>(v));
            else y[(int64_t)(t0 + row) * N + n0 + col] = w8_f32_to_act<ADT>(v);
        }
    }
}

template <int ADT, int BITS, bool GROUPED>
__global__ __launch_bounds__(W8_THREADS) void w8_linear_kernel(const uint16_t* __restrict__ x, int T, const uint8_t* __restrict__ q, int64_t ldq,
                                                              const float* __restrict__ scale, const float* __restrict__ zero,
                                                              const uint16_t* __restrict__ bias, int N, int K, uint16_t* __restrict__ y, int ft,
                                                              int nkfull, int vec, int ng, int gshift) {
    __shared__ float red[W8_WAVES][16 * 64];
    w8_tile<ADT, BITS, GROUPED, false, false>(red, x, T, q, ldq, scale, zero, bias, N, K, y, blockIdx.y * 32, blockIdx.x * ft, ft, nkfull, vec, ng, gshift);
}

// ---- K16: a packed SVDLinear factor pair in one launch --------------------------------------------------------------------------------
//   z[T, r] = fp16( x[T, K] . wB^T )            phase 1, a unit = (token tile, ft1 rows of B)
//   grid barrier (grid <= #CUs: co-resident; bounded spin, give-up word, NaN poison: grid_sync.h)
//   y[T, N] = fp16( z . wA^T + bias )           phase 2, a unit = (token tile, ft2 rows of A)
// Both phases are w8_tile, so every element of z and of y sees the operations of w8_linear_kernel on the same operands (iteration `it` belongs
// to wave it % 4, chunk m to MFMA m, and the order of the LDS reduction does not depend on the workgroup or on ft): the launch returns the
// bits of the two launches it replaces.  z ([round_up(T, 32), r] fp16 behind the 256-byte barrier block of the workspace) is stored and loaded
// at agent scope; rows at or beyond T and nothing else of it stay unwritten and are never read (token rows are clamped as in the tile loop).
// A workgroup takes units blockIdx.x, + gridDim.x, ...; one without a unit in a phase still arrives at the barrier.
template <int ADT, int BITS, bool GROUPED>
__global__ __launch_bounds__(W8_THREADS, 1) void lowrank_packed_kernel(const uint16_t* __restrict__ x, int T, const uint8_t* __restrict__ qB,
                                                                      int64_t ldB, const float* __restrict__ scaleB, const float* __restrict__ zeroB,
                                                                      const uint8_t* __restrict__ qA, int64_t ldA, const float* __restrict__ scaleA,
                                                                      const float* __restrict__ zeroA, const uint16_t* __restrict__ bias, int N, int K,
                                                                      int r, uint16_t* __restrict__ y, uint16_t* z, unsigned* bar, int ft1, int ft2,
                                                                      int gshift) {
    __shared__ float red[W8_WAVES][16 * 64];
    const int nT = (T + 31) / 32, G = gridDim.x;
    const int ns1 = (r + ft1 - 1) / ft1, ns2 = (N + ft2 - 1) / ft2;
    const int ngB = GROUPED ? (K + (1 << gshift) - 1) >> gshift : 1, ngA = GROUPED ? (r + (1 << gshift) - 1) >> gshift : 1;

    for (int u = blockIdx.x; u < nT * ns1; u += G) {
        w8_tile<ADT, BITS, GROUPED, false, true>(red, x, T, qB, ldB, scaleB, zeroB, nullptr, r, K, z, (u / ns1) * 32, (u % ns1) * ft1, ft1, K / W8_KIT, 1,
                                            ngB, gshift);
        __syncthreads();
    }

    grid_barrier(bar, (unsigned)G);

    for (int u = blockIdx.x; u < nT * ns2; u += G) {
        w8_tile<ADT, BITS, GROUPED, true, false>(red, z, T, qA, ldA, scaleA, zeroA, bias, N, r, y, (u / ns2) * 32, (u % ns2) * ft2, ft2, r / W8_KIT, 1,
                                            ngA, gshift);
        __syncthreads();
    }
    if (gave_up(bar))   // poison this workgroup's own tiles
        for (int u = blockIdx.x; u < nT * ns2; u += G) {
            const int t0 = (u / ns2) * 32, n0 = (u % ns2) * ft2, nvalid = min(ft2, N - n0);
            for (int e = threadIdx.x; e < 1024; e += W8_THREADS) {
                const int row = e >> 5, col = e & 31;
                if (col < nvalid && t0 + row < T) y[(int64_t)(t0 + row) * N + n0 + col] = W8_ACT_NAN<ADT>;
            }
        }
}

// ---- K17: a token-tiled GEMM on the packed codes, for inputs beyond decode ---------------------------------------------------------------
// A workgroup owns BM = 32 MS tokens x BN = 32 MS features of y, MS = 4, 2 or 1 (pg_sub_tiles picks the widest that still fills the chip).  Its
// four waves are MS feature groups (a wave owns 32 WHOLE features) times WGK = 4 / MS k groups: wave (wn, kg) takes the k steps of 128 with
// step % WGK == kg.  Per "super-step" of WGK steps the workgroup stages x[BM, 128 WGK] ONCE through LDS (always 128 LDS rows of 256 bytes =
// 32 KB: row kg BM + r holds token r's 128 values of k group kg), plain 16-byte loads in full 256-byte row segments and ds_write_b128, two
// buffers: the loads of super-step s + 1 are in flight under the MFMAs of s, one barrier per super-step.  Codes do not go through LDS: lane
// (i, g) loads row i's 64-code block of its step with the loads of w8_iter_load, dequantizes it ONCE (w8_chunk_f16: the fake quantizer's value)
// and reuses the eight operands for the MS 32-token sub-tiles, whose x operands it reads from LDS (ds_read_b128); both operands carry the
// k permutation of the decode kernel (chunk m of the lane's block to MFMAs 2 m, 2 m + 1).
// LDS image: 16-byte slot c of LDS row R sits at slot c ^ (R & 15).  A ds_read_b128 is served in groups of 16 lanes that here hold 16 rows
// with pairwise different R & 15 and one column c: unswizzled that is one 4-bank column (16-way conflict), swizzled 16 different slots.
// Edges: token rows at or beyond T and feature rows at or beyond N re-read the last valid row and are not stored; beyond K BOTH operands are
// zero (x slots are staged as zeros, code chunks are masked), and a step that lies wholly beyond K is skipped.
// Order of the sums: a wave adds its steps in ascending k; the WGK partial tiles are added in ascending kg through LDS (the staging buffers,
// free after the last barrier), by the kg = 0 wave, which adds the bias and stores.  No atomics; nothing depends on timing.
constexpr int PG_LDS_ROWS = 128;                     // LDS rows (256 bytes: 128 fp16) of one staged x tile
constexpr int PG_TILE_SLOTS = PG_LDS_ROWS * 16;      // 16-byte slots of one tile
constexpr int PG_STAGE = PG_TILE_SLOTS / W8_THREADS; // slots a thread stages per super-step

// the lane's 64-code block of step `it` and, GROUPED, its scale and zero.  whole: the step lies within K (unconditional loads)
template <int BITS, bool GROUPED>
__device__ __forceinline__ void pg_load_codes(uint4 (&cv)[W8_CW<BITS>], float& sc, float& zr, const uint8_t* __restrict__ qrow,
                                              const float* __restrict__ srow, const float* __restrict__ zrow, int it, int g, int K, int ng, int gshift,
                                              bool whole) {
    const uint4* cp = (const uint4*)(qrow + (int64_t)it * (W8_KIT * BITS / 8));
    const int k0 = it * W8_KIT + 64 * g;
    if (whole) {
#pragma unroll
        for (int m = 0; m < W8_CW<BITS>; ++m) cv[m] = cp[m];
        if constexpr (GROUPED) sc = srow[k0 >> gshift], zr = zrow[k0 >> gshift];
    } else {
        // BITS 8: 16-byte word m is chunk m, there when it starts below K (K % 16 == 0).  BITS 6, 4: rows are padded to whole blocks
#pragma unroll
        for (int m = 0; m < W8_CW<BITS>; ++m) cv[m] = (BITS == 8 ? k0 + 16 * m : k0) < K ? cp[m] : make_uint4(0, 0, 0, 0);
        if constexpr (GROUPED) {   // a block that starts at or beyond K has no group: the row's last pair, every chunk of it is masked
            const int gi = min(k0 >> gshift, ng - 1);
            sc = srow[gi], zr = zrow[gi];
        }
    }
}

// one step of a wave: dequantize the lane's block, and for each of the MS token sub-tiles the 8 MFMAs on the x operands of LDS rows
// row0 + 32 s + i (row0 = kg BM).  MASK: the step crosses K, chunks at or beyond K are zero
template <int ADT, int BITS, int MS, bool MASK>
__device__ __forceinline__ void pg_step(f32x16 (&acc)[MS], const uint4 (&cv)[W8_CW<BITS>], float sc, float zr, const uint4* __restrict__ tile, int row0,
                                        int i, int g, int kleft /* K - first k of the lane's block */) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        uint32_t w[W8_CW<BITS>];
        uint4 w0, w1;
        w8_chunk_words<BITS>(cv, m, w);
        w8_chunk_f16<ADT, BITS, MASK>(w, sc, zr, MASK ? max(0, min(16, kleft - 16 * m)) : 16, w0, w1);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int s = 0; s < MS; ++s) {
                const uint4 xa = tile[(row0 + 32 * s + i) * 16 + ((8 * g + 2 * m + h) ^ (i & 15))];
                acc[s] = w8_mfma<ADT>(xa, h ? w1 : w0, acc[s]);
            }
    }
}

template <int ADT, int BITS, bool GROUPED, int MS>
__global__ __launch_bounds__(W8_THREADS, 2) void packed_gemm_kernel(const uint16_t* __restrict__ x, int T, const uint8_t* __restrict__ q, int64_t ldq,
                                                                   const float* __restrict__ scale, const float* __restrict__ zero,
                                                                   const uint16_t* __restrict__ bias, int N, int K, uint16_t* __restrict__ y, int ng,
                                                                   int gshift) {
    constexpr int WGK = W8_WAVES / MS, BM = 32 * MS, BN = 32 * MS;
    __shared__ uint4 lds[2 * PG_TILE_SLOTS];   // ALL the LDS of the kernel: the two x tiles, then the partial tiles of the k groups (64 KB)
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int i = lane & 31, g = lane >> 5;
    const int wn = wave % MS, kg = wave / MS;
    const int t0 = blockIdx.y * BM, n0 = blockIdx.x * BN + 32 * wn;
    const int wrow = min(n0 + i, N - 1);
    const uint8_t* qrow = q + (int64_t)wrow * ldq + 8 * BITS * g;
    const float* srow = scale + (GROUPED ? (int64_t)wrow * ng : 0);
    const float* zrow = zero + (GROUPED ? (int64_t)wrow * ng : 0);
    float sc = 0.f, zr = 0.f, scn = 0.f, zrn = 0.f;
    if constexpr (!GROUPED) sc = scn = scale[wrow], zr = zrn = zero[wrow];

    // staging: slot p of the thread is LDS row 16 p + (tid >> 4), column slot tid & 15: 16 threads take one row's 256 bytes
    const int srw = tid >> 4, scol = tid & 15;
    const uint16_t* xsrc[PG_STAGE];   // token row (clamped) and column of every slot, at k group 0 of super-step 0
    int skoff[PG_STAGE];              // first k of the slot within a super-step
#pragma unroll
    for (int p = 0; p < PG_STAGE; ++p) {
        const int R = 16 * p + srw, r = R % BM;
        skoff[p] = (R / BM) * W8_KIT + 8 * scol;
        xsrc[p] = x + (int64_t)min(t0 + r, T - 1) * K + skoff[p];
    }
    const int sdst = srw * 16 + (scol ^ srw);   // (16 p + srw) & 15 == srw

    const int nk = (K + W8_KIT - 1) / W8_KIT, nss = (nk + WGK - 1) / WGK;
    f32x16 acc[MS];
#pragma unroll
    for (int s = 0; s < MS; ++s)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;

    uint4 xs[PG_STAGE], cv[W8_CW<BITS>], cvn[W8_CW<BITS>];
#pragma unroll
    for (int m = 0; m < W8_CW<BITS>; ++m) cv[m] = cvn[m] = make_uint4(0, 0, 0, 0);
    auto stage_load = [&](int ss) {
        const int kb = ss * (WGK * W8_KIT);
        if (kb + WGK * W8_KIT <= K) {   // the whole super-step lies within K: unconditional loads (workgroup-uniform)
#pragma unroll
            for (int p = 0; p < PG_STAGE; ++p) xs[p] = *(const uint4*)(xsrc[p] + kb);
        } else {
#pragma unroll
            for (int p = 0; p < PG_STAGE; ++p) xs[p] = kb + skoff[p] < K ? *(const uint4*)(xsrc[p] + kb) : make_uint4(0, 0, 0, 0);   // K % 8 == 0
        }
    };
    auto stage_write = [&](int buf) {
#pragma unroll
        for (int p = 0; p < PG_STAGE; ++p) lds[buf * PG_TILE_SLOTS + 256 * p + sdst] = xs[p];
    };

    stage_load(0);
    if (kg < nk) pg_load_codes<BITS, GROUPED>(cv, sc, zr, qrow, srow, zrow, kg, g, K, ng, gshift, (kg + 1) * W8_KIT <= K);
    stage_write(0);
    __syncthreads();
    for (int ss = 0; ss < nss; ++ss) {
        const int it = ss * WGK + kg, itn = it + WGK;
        if (ss + 1 < nss) stage_load(ss + 1);
        if (itn < nk) pg_load_codes<BITS, GROUPED>(cvn, scn, zrn, qrow, srow, zrow, itn, g, K, ng, gshift, (itn + 1) * W8_KIT <= K);
        const uint4* tile = lds + (ss & 1) * PG_TILE_SLOTS;
        if ((it + 1) * W8_KIT <= K) pg_step<ADT, BITS, MS, false>(acc, cv, sc, zr, tile, kg * BM, i, g, 64);
        else if (it < nk) pg_step<ADT, BITS, MS, true>(acc, cv, sc, zr, tile, kg * BM, i, g, K - it * W8_KIT - 64 * g);
        if (ss + 1 < nss) stage_write((ss + 1) & 1);   // the buffer of super-step ss - 1: every wave has passed the barrier that ended it
#pragma unroll
        for (int m = 0; m < W8_CW<BITS>; ++m) cv[m] = cvn[m];
        if constexpr (GROUPED) sc = scn, zr = zrn;
        __syncthreads();
    }

    if constexpr (WGK > 1) {   // the partial tiles of k groups 1 .. WGK - 1, added in that order by the k group 0 wave of the same features
        float* red = (float*)lds;
        if (kg > 0) {
#pragma unroll
            for (int s = 0; s < MS; ++s)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[((((kg - 1) * MS + wn) * MS + s) * 16 + r) * 64 + lane] = acc[s][r];
        }
        __syncthreads();
        if (kg == 0) {
#pragma unroll
            for (int k2 = 1; k2 < WGK; ++k2)
#pragma unroll
                for (int s = 0; s < MS; ++s)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[s][r] += red[((((k2 - 1) * MS + wn) * MS + s) * 16 + r) * 64 + lane];
        }
    }
    if (kg == 0 && n0 + i < N) {   // accumulator register r of lane (i, g): token (r & 3) + 8 (r >> 2) + 4 g of the sub-tile, feature i
        const float b = bias ? w8_act_to_f32<ADT>(bias[n0 + i]) : 0.f;
#pragma unroll
        for (int s = 0; s < MS; ++s)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int tok = t0 + 32 * s + (r & 3) + 8 * (r >> 2) + 4 * g;
                if (tok < T) {
                    float v = acc[s][r];
                    if (bias) v += b;
                    y[(int64_t)tok * N + n0 + i] = w8_f32_to_act<ADT>(v);
                }
            }
    }
}

// ---- dequantization to a dense weight ---------------------------------------------------------------------------------------------
// scale / zero are [rows, ng], a group is 1 << gshift columns (per row: ng = 1 and W8_ROW_SHIFT, which sends every column to group 0).  A
// thread's 16 codes start at a multiple of 16 and so share one group
// one thread per 16 consecutive codes of a row, 16-byte loads and stores (cols % 16 == 0, aligned rows)
template <int DT>
__global__ __launch_bounds__(W8_THREADS) void w8_dequant_kernel(const uint8_t* __restrict__ q, int64_t ldq, const float* __restrict__ scale,
                                                               const float* __restrict__ zero, int64_t rows, int64_t cols, void* __restrict__ out,
                                                               int64_t ldo, int64_t ng, int gshift) {
    const int64_t chunks = (cols + 15) / 16;
    const int64_t id = (int64_t)blockIdx.x * W8_THREADS + threadIdx.x;
    if (id >= rows * chunks) return;
    const int64_t row = id / chunks, c0 = (id - row * chunks) * 16;
    const float sc = scale[row * ng + (c0 >> gshift)], zr = zero[row * ng + (c0 >> gshift)];
    const uint8_t* qp = q + row * ldq + c0;
    typename elem<DT>::T* op = (typename elem<DT>::T*)out + row * ldo + c0;
    {
        const uint4 c = *(const uint4*)qp;
        const uint32_t w[4] = {c.x, c.y, c.z, c.w};
        if (DT == ASVD_F32) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                ((uint4*)op)[j] = make_uint4(__float_as_uint(w8_value(w[j] & 0xffu, sc, zr)), __float_as_uint(w8_value((w[j] >> 8) & 0xffu, sc, zr)),
                                             __float_as_uint(w8_value((w[j] >> 16) & 0xffu, sc, zr)), __float_as_uint(w8_value(w[j] >> 24, sc, zr)));
        } else {
            uint32_t h[8];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const float a = w8_value((w[j] >> (16 * p)) & 0xffu, sc, zr), b = w8_value((w[j] >> (16 * p + 8)) & 0xffu, sc, zr);
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
                                                                    void* __restrict__ out, int64_t ldo, int64_t ng, int gshift) {
    const int64_t id = (int64_t)blockIdx.x * W8_THREADS + threadIdx.x;
    if (id >= rows * cols) return;
    const int64_t row = id / cols, c = id - row * cols, si = row * ng + (c >> gshift);
    elem<DT>::st(out, row * ldo + c, w8_value((uint32_t)q[row * ldq + c], scale[si], zero[si]));
}

// ---- codes at their own width: pack and dequantization -----------------------------------------------------------------------------
// bytes of a bitstream row of `cols` codes: whole blocks of 64 codes
__host__ __device__ inline int64_t wb_row_bytes(int64_t cols, int bits) { return (cols + 63) / 64 * 8 * bits; }

// one thread per 16 consecutive codes of a padded row: BITS / 2 words of the bitstream (4-byte stores).  Codes are masked to BITS bits, codes
// at or beyond cols are the padding zeros
template <int BITS>
__global__ __launch_bounds__(W8_THREADS) void wb_pack_kernel(const uint8_t* __restrict__ q, int64_t ldq, int64_t rows, int64_t cols,
                                                            uint8_t* __restrict__ out, int64_t ld_bytes) {
    const int64_t chunks = (cols + 63) / 64 * 4;
    const int64_t id = (int64_t)blockIdx.x * W8_THREADS + threadIdx.x;
    if (id >= rows * chunks) return;
    const int64_t row = id / chunks, c0 = (id - row * chunks) * 16;
    const uint8_t* qp = q + row * ldq + c0;
    uint32_t w[W8_CW<BITS>];
#pragma unroll
    for (int t = 0; t < W8_CW<BITS>; ++t) w[t] = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t code = c0 + j < cols ? (uint32_t)qp[j] & ((1u << BITS) - 1u) : 0u;
        const int bit = BITS * j, lo = bit >> 5, sh = bit & 31;
        w[lo] |= code << sh;
        if (sh + BITS > 32) w[lo + 1 < W8_CW<BITS> ? lo + 1 : lo] |= code >> ((32 - sh) & 31);
    }
    uint32_t* op = (uint32_t*)(out + row * ld_bytes + c0 / 8 * BITS);
#pragma unroll
    for (int t = 0; t < W8_CW<BITS>; ++t) op[t] = w[t];
}

// one thread per 16 consecutive codes of a row (4-byte loads of the bitstream).  vec: whole chunks and an aligned destination, 16-byte stores;
// otherwise element stores, none at or beyond cols
template <int DT, int BITS>
__global__ __launch_bounds__(W8_THREADS) void wb_dequant_kernel(const uint8_t* __restrict__ q, int64_t ld_bytes, const float* __restrict__ scale,
                                                               const float* __restrict__ zero, int64_t rows, int64_t cols, void* __restrict__ out,
                                                               int64_t ldo, int vec, int64_t ng, int gshift) {
    const int64_t chunks = (cols + 15) / 16;
    const int64_t id = (int64_t)blockIdx.x * W8_THREADS + threadIdx.x;
    if (id >= rows * chunks) return;
    const int64_t row = id / chunks, c0 = (id - row * chunks) * 16;
    const float sc = scale[row * ng + (c0 >> gshift)], zr = zero[row * ng + (c0 >> gshift)];
    const uint32_t* qp = (const uint32_t*)(q + row * ld_bytes + c0 / 8 * BITS);
    uint32_t w[W8_CW<BITS>];
#pragma unroll
    for (int t = 0; t < W8_CW<BITS>; ++t) w[t] = qp[t];
    float v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = w8_value(w8_code<BITS>(w, j), sc, zr);
    if (vec) {
        typename elem<DT>::T* op = (typename elem<DT>::T*)out + row * ldo + c0;
        if (DT == ASVD_F32) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                ((uint4*)op)[j] = make_uint4(__float_as_uint(v[4 * j]), __float_as_uint(v[4 * j + 1]), __float_as_uint(v[4 * j + 2]),
                                             __float_as_uint(v[4 * j + 3]));
        } else {
            uint32_t h[8];
#pragma unroll
            for (int p = 0; p < 8; ++p)
                h[p] = DT == ASVD_F16 ? ((uint32_t)f32_to_f16_bits(v[2 * p]) | ((uint32_t)f32_to_f16_bits(v[2 * p + 1]) << 16))
                                      : ((uint32_t)f32_to_bf16_bits(v[2 * p]) | ((uint32_t)f32_to_bf16_bits(v[2 * p + 1]) << 16));
            ((uint4*)op)[0] = make_uint4(h[0], h[1], h[2], h[3]);
            ((uint4*)op)[1] = make_uint4(h[4], h[5], h[6], h[7]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (c0 + j < cols) elem<DT>::st(out, row * ldo + c0 + j, v[j]);
    }
}

// the CU count of the current device.  Per-call host cost matters at decode size: the count of the first W8_MAX_DEVICES devices is looked up once
// (relaxed atomics: two threads may both look it up and store the same value); devices beyond that are asked every call
int w8_cu_count(int* cus_out) {
    static std::atomic<int> s_cus[W8_MAX_DEVICES];
    int dev = 0;
    ASVD_HIP_CHECK(hipGetDevice(&dev));
    int cus = (dev >= 0 && dev < W8_MAX_DEVICES) ? s_cus[dev].load(std::memory_order_relaxed) : 0;
    if (!cus) {
        ASVD_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        if (cus < 1) return ASVD_E_HIP;
        if (dev >= 0 && dev < W8_MAX_DEVICES) s_cus[dev].store(cus, std::memory_order_relaxed);
    }
    *cus_out = cus;
    return ASVD_OK;
}

// the widest feature tile that still puts a workgroup on every CU (bandwidth-bound: more streams win over fuller MFMA tiles)
int w8_feature_tile(int nT, int64_t N, int cus) {
    int ft = 32;
    while (ft > 8 && nT * ceil_div64(N, ft) < cus) ft /= 2;
    return ft;
}

// the activation types of the forward kernels
inline bool w8_act_ok(int adt) { return adt == ASVD_F16 || adt == ASVD_BF16; }

// group: 0 (scale / zero [N]) or 64 / 128 (K14: [N, ceil(K / group)]); the entry points have checked it
template <int ADT>
int w8_linear_go(const void* x, int64_t T, const void* q, int64_t ldq, const float* scale, const float* zero, int group, const void* bias,
                     int64_t N, int64_t K, void* y, void* stream) {
    if (!x || !q || !scale || !zero || !y) return ASVD_E_BADARG;
    if (T < 1 || T > ASVD_W8_MAX_TOKENS || N < 1 || K < 1 || ldq < K || N > 0x7fffffff - 64 || K > 0x7fffffff - 256) return ASVD_E_BADARG;
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)bias) & 1) return ASVD_E_BADARG;   // 2-byte elements
    if (group && (K % 16 || (uintptr_t)x % 16 || (uintptr_t)q % 16 || ldq % 16)) return ASVD_E_BADARG;   // grouped: 16-byte loads only
    int cus = 0;
    const int st = w8_cu_count(&cus);
    if (st != ASVD_OK) return st;
    const int nT = (int)((T + 31) / 32);
    const int ft = w8_feature_tile(nT, N, cus);
    const bool vec = ((uintptr_t)x % 16 == 0) && ((uintptr_t)q % 16 == 0) && (K % 8 == 0) && (ldq % 16 == 0);
    const int nkfull = vec ? (int)(K / W8_KIT) : 0;
    if (group)
        hipLaunchKernelGGL((w8_linear_kernel<ADT, 8, true>), dim3((unsigned)ceil_div64(N, ft), (unsigned)nT), dim3(W8_THREADS), 0, (hipStream_t)stream,
                           (const uint16_t*)x, (int)T, (const uint8_t*)q, ldq, scale, zero, (const uint16_t*)bias, (int)N, (int)K, (uint16_t*)y, ft,
                           nkfull, 1, (int)ceil_div64(K, group), group == 64 ? 6 : 7);
    else
        hipLaunchKernelGGL((w8_linear_kernel<ADT, 8, false>), dim3((unsigned)ceil_div64(N, ft), (unsigned)nT), dim3(W8_THREADS), 0, (hipStream_t)stream,
                           (const uint16_t*)x, (int)T, (const uint8_t*)q, ldq, scale, zero, (const uint16_t*)bias, (int)N, (int)K, (uint16_t*)y, ft,
                           nkfull, vec ? 1 : 0, 1, 0);
    ASVD_HIP_CHECK(hipGetLastError());
    return ASVD_OK;
}

int w8_linear_launch(const void* x, int adt, int64_t T, const void* q, int64_t ldq, const float* scale, const float* zero, int group, const void* bias,
                     int64_t N, int64_t K, void* y, void* stream) {
    if (!w8_act_ok(adt)) return ASVD_E_BADARG;
    return adt == ASVD_BF16 ? w8_linear_go<ASVD_BF16>(x, T, q, ldq, scale, zero, group, bias, N, K, y, stream)
                            : w8_linear_go<ASVD_F16>(x, T, q, ldq, scale, zero, group, bias, N, K, y, stream);
}

int w8_dequant_launch(const void* q, int64_t ldq, const float* scale, const float* zero, int group, int64_t rows, int64_t cols, void* out,
                      int out_dtype, int64_t ldo, void* stream) {
    const int64_t ng = group ? ceil_div64(cols, group) : 1;
    const int gshift = group == 64 ? 6 : group == 128 ? 7 : W8_ROW_SHIFT;
    if (!q || !scale || !zero || !out || rows < 1 || cols < 1 || ldq < cols || ldo < cols || !dtype_ok(out_dtype)) return ASVD_E_BADARG;
    const int64_t es = (int64_t)dtype_size(out_dtype);
    if ((uintptr_t)out % es) return ASVD_E_BADARG;
    const bool vec_ok = (cols % 16 == 0) && ((uintptr_t)q % 16 == 0) && (ldq % 16 == 0) && ((uintptr_t)out % 16 == 0) && ((ldo * es) % 16 == 0);
    const int64_t grid = ceil_div64(vec_ok ? rows * (cols / 16) : rows * cols, W8_THREADS);
    if (grid > 0x7fffffff) return ASVD_E_BADARG;
    if (vec_ok) {
        ASVD_DISPATCH_DTYPE(out_dtype, DT,
                            hipLaunchKernelGGL(w8_dequant_kernel<DT>, dim3((unsigned)grid), dim3(W8_THREADS), 0, (hipStream_t)stream, (const uint8_t*)q,
                                               ldq, scale, zero, rows, cols, out, ldo, ng, gshift));
    } else {
        ASVD_DISPATCH_DTYPE(out_dtype, DT,
                            hipLaunchKernelGGL(w8_dequant_elem_kernel<DT>, dim3((unsigned)grid), dim3(W8_THREADS), 0, (hipStream_t)stream,
                                               (const uint8_t*)q, ldq, scale, zero, rows, cols, out, ldo, ng, gshift));
    }
    ASVD_HIP_CHECK(hipGetLastError());
    return ASVD_OK;
}

int wb_dequant_launch(const void* q, int64_t ld_bytes, int bits, const float* scale, const float* zero, int group, int64_t rows, int64_t cols,
                      void* out, int out_dtype, int64_t ldo, void* stream) {
    const int64_t ng = group ? ceil_div64(cols, group) : 1;
    const int gshift = group == 64 ? 6 : group == 128 ? 7 : W8_ROW_SHIFT;
    if (!q || !scale || !zero || !out || rows < 1 || cols < 1 || ldo < cols || !dtype_ok(out_dtype) || (bits != 4 && bits != 6)) return ASVD_E_BADARG;
    if (ld_bytes < wb_row_bytes(cols, bits) || (uintptr_t)q % 4 || ld_bytes % 4) return ASVD_E_BADARG;   // 4-byte loads
    const int64_t es = (int64_t)dtype_size(out_dtype);
    if ((uintptr_t)out % es) return ASVD_E_BADARG;
    const int vec = (cols % 16 == 0) && ((uintptr_t)out % 16 == 0) && ((ldo * es) % 16 == 0);
    const int64_t grid = ceil_div64(rows * ((cols + 15) / 16), W8_THREADS);
    if (grid > 0x7fffffff) return ASVD_E_BADARG;
    if (bits == 6) {
        ASVD_DISPATCH_DTYPE(out_dtype, DT,
                            hipLaunchKernelGGL((wb_dequant_kernel<DT, 6>), dim3((unsigned)grid), dim3(W8_THREADS), 0, (hipStream_t)stream,
                                               (const uint8_t*)q, ld_bytes, scale, zero, rows, cols, out, ldo, vec, ng, gshift));
    } else {
        ASVD_DISPATCH_DTYPE(out_dtype, DT,
                            hipLaunchKernelGGL((wb_dequant_kernel<DT, 4>), dim3((unsigned)grid), dim3(W8_THREADS), 0, (hipStream_t)stream,
                                               (const uint8_t*)q, ld_bytes, scale, zero, rows, cols, out, ldo, vec, ng, gshift));
    }
    ASVD_HIP_CHECK(hipGetLastError());
    return ASVD_OK;
}

template <int ADT>
int wb_linear_go(const void* x, int64_t T, const void* q, int64_t ld_bytes, int bits, const float* scale, const float* zero, int group,
                     const void* bias, int64_t N, int64_t K, void* y, void* stream) {
    if (!x || !q || !scale || !zero || !y || (bits != 4 && bits != 6)) return ASVD_E_BADARG;
    if (T < 1 || T > ASVD_W8_MAX_TOKENS || N < 1 || K < 1 || K % 16 || N > 0x7fffffff - 64 || K > 0x7fffffff - 256) return ASVD_E_BADARG;
    if (ld_bytes < wb_row_bytes(K, bits) || ld_bytes % 16 || (uintptr_t)x % 16 || (uintptr_t)q % 16) return ASVD_E_BADARG;   // 16-byte loads only
    if (((uintptr_t)y | (uintptr_t)bias) & 1) return ASVD_E_BADARG;   // 2-byte elements
    int cus = 0;
    const int st = w8_cu_count(&cus);
    if (st != ASVD_OK) return st;
    const int nT = (int)((T + 31) / 32);
    const int ft = w8_feature_tile(nT, N, cus);
    const dim3 grid((unsigned)ceil_div64(N, ft), (unsigned)nT);
    const int ng = group ? (int)ceil_div64(K, group) : 1, gshift = group == 64 ? 6 : 7;
    if (group && bits == 6)
        hipLaunchKernelGGL((w8_linear_kernel<ADT, 6, true>), grid, dim3(W8_THREADS), 0, (hipStream_t)stream, (const uint16_t*)x, (int)T, (const uint8_t*)q,
                           ld_bytes, scale, zero, (const uint16_t*)bias, (int)N, (int)K, (uint16_t*)y, ft, (int)(K / W8_KIT), 1, ng, gshift);
    else if (group)
        hipLaunchKernelGGL((w8_linear_kernel<ADT, 4, true>), grid, dim3(W8_THREADS), 0, (hipStream_t)stream, (const uint16_t*)x, (int)T, (const uint8_t*)q,
                           ld_bytes, scale, zero, (const uint16_t*)bias, (int)N, (int)K, (uint16_t*)y, ft, (int)(K / W8_KIT), 1, ng, gshift);
    else if (bits == 6)
        hipLaunchKernelGGL((w8_linear_kernel<ADT, 6, false>), grid, dim3(W8_THREADS), 0, (hipStream_t)stream, (const uint16_t*)x, (int)T, (const uint8_t*)q,
                           ld_bytes, scale, zero, (const uint16_t*)bias, (int)N, (int)K, (uint16_t*)y, ft, (int)(K / W8_KIT), 1, 1, 0);
    else
        hipLaunchKernelGGL((w8_linear_kernel<ADT, 4, false>), grid, dim3(W8_THREADS), 0, (hipStream_t)stream, (const uint16_t*)x, (int)T, (const uint8_t*)q,
                           ld_bytes, scale, zero, (const uint16_t*)bias, (int)N, (int)K, (uint16_t*)y, ft, (int)(K / W8_KIT), 1, 1, 0);
    ASVD_HIP_CHECK(hipGetLastError());
    return ASVD_OK;
}

int wb_linear_launch(const void* x, int adt, int64_t T, const void* q, int64_t ld_bytes, int bits, const float* scale, const float* zero, int group,
                     const void* bias, int64_t N, int64_t K, void* y, void* stream) {
    if (!w8_act_ok(adt)) return ASVD_E_BADARG;
    return adt == ASVD_BF16 ? wb_linear_go<ASVD_BF16>(x, T, q, ld_bytes, bits, scale, zero, group, bias, N, K, y, stream)
                            : wb_linear_go<ASVD_F16>(x, T, q, ld_bytes, bits, scale, zero, group, bias, N, K, y, stream);
}

template <int ADT, int BITS, bool GROUPED>
void lowrank_packed_go(int grid, hipStream_t stream, const void* x, int64_t T, const void* qB, int64_t ldB, const float* scaleB, const float* zeroB,
                       const void* qA, int64_t ldA, const float* scaleA, const float* zeroA, const void* bias, int64_t N, int64_t K, int64_t r, void* y,
                       void* work, int ft1, int ft2, int gshift) {
    hipLaunchKernelGGL((lowrank_packed_kernel<ADT, BITS, GROUPED>), dim3((unsigned)grid), dim3(W8_THREADS), 0, stream, (const uint16_t*)x, (int)T,
                       (const uint8_t*)qB, ldB, scaleB, zeroB, (const uint8_t*)qA, ldA, scaleA, zeroA, (const uint16_t*)bias, (int)N, (int)K, (int)r,
                       (uint16_t*)y, (uint16_t*)((char*)work + 256), (unsigned*)work, ft1, ft2, gshift);
}

// K17: the widest tile (32 MS tokens x 32 MS features, MS = 4, 2, 1) that the token count fills and that still puts a workgroup on every
// other CU; below that the tile narrows and the k steps spread over the 4 / MS wave groups of more workgroups instead
int pg_sub_tiles(int64_t T, int64_t N, int cus) {
    for (int ms = 4; ms > 1; ms /= 2)
        if (T > 16 * ms && ceil_div64(T, 32 * ms) * ceil_div64(N, 32 * ms) * 2 >= cus) return ms;
    return 1;
}

template <int ADT, int BITS, bool GROUPED>
void pg_go(int ms, hipStream_t stream, const void* x, int64_t T, const void* q, int64_t ldq, const float* scale, const float* zero, const void* bias,
           int64_t N, int64_t K, void* y, int ng, int gshift) {
    const dim3 grid((unsigned)ceil_div64(N, 32 * ms), (unsigned)ceil_div64(T, 32 * ms));
#define ASVD_PG_LAUNCH(MS) hipLaunchKernelGGL((packed_gemm_kernel<ADT, BITS, GROUPED, MS>), grid, dim3(W8_THREADS), 0, stream, (const uint16_t*)x, (int)T, \
                                              (const uint8_t*)q, ldq, scale, zero, (const uint16_t*)bias, (int)N, (int)K, (uint16_t*)y, ng, gshift)
    if (ms == 4) ASVD_PG_LAUNCH(4);
    else if (ms == 2) ASVD_PG_LAUNCH(2);
    else ASVD_PG_LAUNCH(1);
#undef ASVD_PG_LAUNCH
}

}  // namespace

extern "C" {

size_t asvd_lowrank_packed_work_bytes(int64_t T, int64_t r) {
    // [barrier: 256 bytes][z: 32 * ceil(T / 32) x r fp16 or bf16]
    return 256 + (size_t)(round_up64(T, 32) * r) * sizeof(uint16_t);
}

int asvd_lowrank_packed_a16(const void* x, int act_dtype, int64_t T, const void* qB, int64_t ldB, const float* scaleB, const float* zeroB,
                            const void* qA, int64_t ldA, const float* scaleA, const float* zeroA, int bits, int64_t group, const void* bias, int64_t N,
                            int64_t K, int64_t r, void* y, void* work, size_t work_bytes, void* stream) {
    if (!w8_act_ok(act_dtype)) return ASVD_E_BADARG;
    if (!x || !qB || !scaleB || !zeroB || !qA || !scaleA || !zeroA || !y || !work) return ASVD_E_BADARG;
    if (T < 1 || T > ASVD_W8_MAX_TOKENS || (bits != 8 && bits != 6 && bits != 4) || (group != 0 && group != 64 && group != 128)) return ASVD_E_BADARG;
    if (N < 1 || K < 1 || r < 1 || K % 16 || r % 16 || N > 0x7fffffff - 64 || K > 0x7fffffff - 256 || r > 0x7fffffff - 256) return ASVD_E_BADARG;
    if (((uintptr_t)x | (uintptr_t)qB | (uintptr_t)qA | (uintptr_t)work) % 16 || ldB % 16 || ldA % 16) return ASVD_E_BADARG;   // 16-byte loads only
    if (ldB < (bits == 8 ? K : wb_row_bytes(K, bits)) || ldA < (bits == 8 ? r : wb_row_bytes(r, bits))) return ASVD_E_BADARG;
    if (((uintptr_t)y | (uintptr_t)bias) & 1) return ASVD_E_BADARG;   // 2-byte elements
    if (work_bytes < asvd_lowrank_packed_work_bytes(T, r)) return ASVD_E_WORKSPACE;
    int cus = 0;
    const int st = w8_cu_count(&cus);
    if (st != ASVD_OK) return st;
    const int nT = (int)((T + 31) / 32);
    const int ft1 = w8_feature_tile(nT, r, cus), ft2 = w8_feature_tile(nT, N, cus);
    const int64_t units1 = nT * ceil_div64(r, ft1), units2 = nT * ceil_div64(N, ft2), units = units1 > units2 ? units1 : units2;
    const int grid = (int)(units < cus ? units : cus);   // <= one workgroup per CU: co-resident, the in-kernel barrier cannot deadlock
    const int gshift = group == 64 ? 6 : 7;
#define ASVD_LRP_GO(B, GR)                                                                                                                          \
    do {                                                                                                                                            \
        if (act_dtype == ASVD_BF16)                                                                                                                 \
            lowrank_packed_go<ASVD_BF16, B, GR>(grid, (hipStream_t)stream, x, T, qB, ldB, scaleB, zeroB, qA, ldA, scaleA, zeroA, bias, N, K, r, y, work, \
                                                ft1, ft2, gshift);                                                                                  \
        else                                                                                                                                        \
            lowrank_packed_go<ASVD_F16, B, GR>(grid, (hipStream_t)stream, x, T, qB, ldB, scaleB, zeroB, qA, ldA, scaleA, zeroA, bias, N, K, r, y, work, \
                                               ft1, ft2, gshift);                                                                                   \
    } while (0)
    if (group) {
        if (bits == 8) ASVD_LRP_GO(8, true);
        else if (bits == 6) ASVD_LRP_GO(6, true);
        else ASVD_LRP_GO(4, true);
    } else {
        if (bits == 8) ASVD_LRP_GO(8, false);
        else if (bits == 6) ASVD_LRP_GO(6, false);
        else ASVD_LRP_GO(4, false);
    }
#undef ASVD_LRP_GO
    ASVD_HIP_CHECK(hipGetLastError());
    return ASVD_OK;
}

int asvd_lowrank_packed_f16(const void* x, int64_t T, const void* qB, int64_t ldB, const float* scaleB, const float* zeroB, const void* qA,
                            int64_t ldA, const float* scaleA, const float* zeroA, int bits, int64_t group, const void* bias, int64_t N, int64_t K,
                            int64_t r, void* y, void* work, size_t work_bytes, void* stream) {
    return asvd_lowrank_packed_a16(x, ASVD_F16, T, qB, ldB, scaleB, zeroB, qA, ldA, scaleA, zeroA, bits, group, bias, N, K, r, y, work, work_bytes,
                                   stream);
}

int64_t asvd_w8_linear_max_tokens(void) { return ASVD_W8_MAX_TOKENS; }

int asvd_w8_linear_f16(const void* x, int64_t T, const void* q, int64_t ldq, const float* scale, const float* zero, const void* bias, int64_t N,
                       int64_t K, void* y, void* stream) {
    return w8_linear_launch(x, ASVD_F16, T, q, ldq, scale, zero, 0, bias, N, K, y, stream);
}

int asvd_w8_linear_grouped_f16(const void* x, int64_t T, const void* q, int64_t ldq, const float* scale, const float* zero, int64_t group,
                               const void* bias, int64_t N, int64_t K, void* y, void* stream) {
    if (group != 64 && group != 128) return ASVD_E_BADARG;
    return w8_linear_launch(x, ASVD_F16, T, q, ldq, scale, zero, (int)group, bias, N, K, y, stream);
}

int asvd_w8_linear_a16(const void* x, int act_dtype, int64_t T, const void* q, int64_t ldq, const float* scale, const float* zero, int64_t group,
                       const void* bias, int64_t N, int64_t K, void* y, void* stream) {
    if (group != 0 && group != 64 && group != 128) return ASVD_E_BADARG;
    return w8_linear_launch(x, act_dtype, T, q, ldq, scale, zero, (int)group, bias, N, K, y, stream);
}

int asvd_w8_dequant(const void* q, int64_t ldq, const float* scale, const float* zero, int64_t rows, int64_t cols, void* out, int out_dtype,
                    int64_t ldo, void* stream) {
    return w8_dequant_launch(q, ldq, scale, zero, 0, rows, cols, out, out_dtype, ldo, stream);
}

int asvd_w8_dequant_grouped(const void* q, int64_t ldq, const float* scale, const float* zero, int64_t group, int64_t rows, int64_t cols, void* out,
                            int out_dtype, int64_t ldo, void* stream) {
    if (group != 64 && group != 128) return ASVD_E_BADARG;
    return w8_dequant_launch(q, ldq, scale, zero, (int)group, rows, cols, out, out_dtype, ldo, stream);
}

int64_t asvd_wb_row_bytes(int64_t cols, int bits) { return (cols < 1 || (bits != 4 && bits != 6)) ? -1 : wb_row_bytes(cols, bits); }

int asvd_wb_pack(const void* q, int64_t ldq, int64_t rows, int64_t cols, int bits, void* out, int64_t ld_bytes, void* stream) {
    if (!q || !out || rows < 1 || cols < 1 || ldq < cols || (bits != 4 && bits != 6)) return ASVD_E_BADARG;
    if (ld_bytes < wb_row_bytes(cols, bits) || (uintptr_t)out % 4 || ld_bytes % 4) return ASVD_E_BADARG;   // 4-byte stores
    const int64_t grid = ceil_div64(rows * ((cols + 63) / 64 * 4), W8_THREADS);
    if (grid > 0x7fffffff) return ASVD_E_BADARG;
    if (bits == 6)
        hipLaunchKernelGGL(wb_pack_kernel<6>, dim3((unsigned)grid), dim3(W8_THREADS), 0, (hipStream_t)stream, (const uint8_t*)q, ldq, rows, cols,
                           (uint8_t*)out, ld_bytes);
    else
        hipLaunchKernelGGL(wb_pack_kernel<4>, dim3((unsigned)grid), dim3(W8_THREADS), 0, (hipStream_t)stream, (const uint8_t*)q, ldq, rows, cols,
                           (uint8_t*)out, ld_bytes);
    ASVD_HIP_CHECK(hipGetLastError());
    return ASVD_OK;
}

int asvd_wb_dequant(const void* q, int64_t ld_bytes, int bits, const float* scale, const float* zero, int64_t rows, int64_t cols, void* out,
                    int out_dtype, int64_t ldo, void* stream) {
    return wb_dequant_launch(q, ld_bytes, bits, scale, zero, 0, rows, cols, out, out_dtype, ldo, stream);
}

int asvd_wb_dequant_grouped(const void* q, int64_t ld_bytes, int bits, const float* scale, const float* zero, int64_t group, int64_t rows,
                            int64_t cols, void* out, int out_dtype, int64_t ldo, void* stream) {
    if (group != 64 && group != 128) return ASVD_E_BADARG;
    return wb_dequant_launch(q, ld_bytes, bits, scale, zero, (int)group, rows, cols, out, out_dtype, ldo, stream);
}

int asvd_wb_linear_f16(const void* x, int64_t T, const void* q, int64_t ld_bytes, int bits, const float* scale, const float* zero, const void* bias,
                       int64_t N, int64_t K, void* y, void* stream) {
    return wb_linear_launch(x, ASVD_F16, T, q, ld_bytes, bits, scale, zero, 0, bias, N, K, y, stream);
}

int asvd_wb_linear_grouped_f16(const void* x, int64_t T, const void* q, int64_t ld_bytes, int bits, const float* scale, const float* zero,
                               int64_t group, const void* bias, int64_t N, int64_t K, void* y, void* stream) {
    if (group != 64 && group != 128) return ASVD_E_BADARG;
    return wb_linear_launch(x, ASVD_F16, T, q, ld_bytes, bits, scale, zero, (int)group, bias, N, K, y, stream);
}

int asvd_wb_linear_a16(const void* x, int act_dtype, int64_t T, const void* q, int64_t ld_bytes, int bits, const float* scale, const float* zero,
                       int64_t group, const void* bias, int64_t N, int64_t K, void* y, void* stream) {
    if (group != 0 && group != 64 && group != 128) return ASVD_E_BADARG;
    return wb_linear_launch(x, act_dtype, T, q, ld_bytes, bits, scale, zero, (int)group, bias, N, K, y, stream);
}

int64_t asvd_packed_gemm_max_tokens(void) { return ASVD_PACKED_GEMM_MAX_TOKENS; }

int asvd_packed_gemm_a16(const void* x, int act_dtype, int64_t T, const void* q, int64_t ld_bytes, int bits, const float* scale, const float* zero,
                         int64_t group, const void* bias, int64_t N, int64_t K, void* y, void* stream) {
    if (!w8_act_ok(act_dtype)) return ASVD_E_BADARG;
    if (!x || !q || !scale || !zero || !y) return ASVD_E_BADARG;
    if ((bits != 8 && bits != 6 && bits != 4) || (group != 0 && group != 64 && group != 128)) return ASVD_E_BADARG;
    if (T < 1 || T > ASVD_PACKED_GEMM_MAX_TOKENS || N < 1 || K < 1 || K % 16 || N > 0x7fffffff - 128 || K > 0x7fffffff - 512) return ASVD_E_BADARG;
    if (ld_bytes < (bits == 8 ? K : wb_row_bytes(K, bits)) || ld_bytes % 16 || (uintptr_t)x % 16 || (uintptr_t)q % 16) return ASVD_E_BADARG;   // 16-byte loads only
    if (((uintptr_t)y | (uintptr_t)bias) & 1) return ASVD_E_BADARG;   // 2-byte elements
    int cus = 0;
    const int st = w8_cu_count(&cus);
    if (st != ASVD_OK) return st;
    const int ms = pg_sub_tiles(T, N, cus);
    const int ng = group ? (int)ceil_div64(K, group) : 1, gshift = group == 64 ? 6 : 7;
#define ASVD_PG_GO(B, GR)                                                                                                         \
    do {                                                                                                                          \
        if (act_dtype == ASVD_BF16) pg_go<ASVD_BF16, B, GR>(ms, (hipStream_t)stream, x, T, q, ld_bytes, scale, zero, bias, N, K, y, ng, gshift); \
        else pg_go<ASVD_F16, B, GR>(ms, (hipStream_t)stream, x, T, q, ld_bytes, scale, zero, bias, N, K, y, ng, gshift);              \
    } while (0)
    if (group) {
        if (bits == 8) ASVD_PG_GO(8, true);
        else if (bits == 6) ASVD_PG_GO(6, true);
        else ASVD_PG_GO(4, true);
    } else {
        if (bits == 8) ASVD_PG_GO(8, false);
        else if (bits == 6) ASVD_PG_GO(6, false);
        else ASVD_PG_GO(4, false);
    }
#undef ASVD_PG_GO
    ASVD_HIP_CHECK(hipGetLastError());
    return ASVD_OK;
}

int asvd_packed_gemm_f16(const void* x, int64_t T, const void* q, int64_t ld_bytes, int bits, const float* scale, const float* zero, int64_t group,
                         const void* bias, int64_t N, int64_t K, void* y, void* stream) {
    return asvd_packed_gemm_a16(x, ASVD_F16, T, q, ld_bytes, bits, scale, zero, group, bias, N, K, y, stream);
}

}  // extern "C"
