// rtn_quant.hip — K11: round-to-nearest (RTN) fake quantization of weights, one pass over HBM per row.
// Replaces quantization.py:17-21,31-140 (Quantizer with perchannel=True, sym=False, mse=False) as rtn_quant_sequential
// (:157-175) applies it: per output row, in fp32,
//   xmin = min(min(row), 0), xmax = max(max(row), 0); both 0 -> -1 / +1; scale = (xmax - xmin) / maxq; zero = round(-xmin / scale)
//   q = clamp(round(x / scale) + zero, 0, maxq); out = scale * (q - zero), rounded once (RNE) to the weight dtype.
// The arithmetic is the reference's op for op: IEEE fp32 division (hipcc's default, no fast-math), rintf (round half to even),
// fp32 denormals kept, min / max that propagate NaN (torch.min / torch.max / torch.clamp do; fminf / fmaxf drop NaN).  Every
// step is a separate rounding: floating-point contraction is off for the whole file (see the pragma below).
//
// A row is read once into registers (16-byte vectors, up to RTN_NV per thread), min/max-reduced, quantized and written once.  Rows of
// up to 64 x RTN_NV vectors (4096 fp16 / bf16, 2048 fp32 elements: every ALinear / BLinear and the 4096-wide projections) take one
// wave each, four to a workgroup, reduced with shuffles alone; longer rows take a workgroup of 256 threads (up to 16384 fp16 / 8192
// fp32 elements); longer still, a two-pass path (reduce, then re-read and write).  The tensors of one launch are described by a
// table that travels in the kernel-argument segment; the workgroups of all of them form one 1-D grid.
//
// K15: the clip search of the reference's Quantizer (quantization.py:94-111, mse=True) is a second instantiation of the kernel.  Between the
// reduction and the final pass it tries `ncand` shrunk ranges p * [xmin, xmax], p = 1 - i / grid, and keeps the (scale, zero) of the smallest
// sum |q(x) - x|^norm over the unit; the unit stays in registers meanwhile.  The candidate pairs are the reference's op for op; the error of a
// candidate is evaluated with a reciprocal, v_log_f32 / v_exp_f32 and a fixed summation order (DPP within 16 lanes, shuffles across a wave, LDS in
// wave order across a workgroup).  With groups, the search kernel gives a group 8 or 16 lanes instead of a wave, so that 4 or 8 groups share a wave.
#include "common.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

// hipcc contracts by default; every operation of this file must round on its own, as the reference's torch ops do
#pragma clang fp contract(off)

namespace {

constexpr int RTN_THREADS = 256;
constexpr int RTN_NV = 8;            // 16-byte vectors held per thread on the register-resident path
constexpr int RTN_MAX_BATCH = 16;    // tensors per launch (table size); longer batches take several launches

struct RtnTensor {
    const void* in;
    void* out;
    float* scale;      // [rows] ([rows, ng] when grouped) or NULL
    float* zero;       // likewise
    uint8_t* codes;    // [rows, cols] contiguous or NULL
    int* flag;         // OR-ed with 1 when a row's scale is 0
    int64_t row0;      // first workgroup of this tensor
    int64_t rows, cols, ldi, ldo;
    int dtype;
    int vec_ok;        // in / out rows 16-byte aligned and cols a multiple of the vector width
    int resident;      // the row fits the registers of its threads
    int per_wave;      // one wave per row (else one workgroup per row)
    int group;         // K14: 0, or the group size (64 / 128): the unit of work is (row, group) and always takes one wave
    int64_t ng;        // groups per row, ceil(cols / group)
};

struct RtnTable {
    RtnTensor t[RTN_MAX_BATCH];
    int n;
    float maxq;
    // K15 (read by the search kernel only)
    float norm;
    int grid;
    int ncand;
};

constexpr int RTN_MAX_CAND = 256;

__device__ __forceinline__ float nan_min(float a, float b) { return (a != a || a < b) ? a : b; }
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || a > b) ? a : b; }

template <int DT> struct rtn_vec { static constexpr int VEC = 8; };
template <> struct rtn_vec<ASVD_F32> { static constexpr int VEC = 4; };

// element k of a 16-byte vector held as four 32-bit words
template <int DT>
__device__ __forceinline__ float vget(const uint4& r, int k) {
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
    if (DT == ASVD_F32) return __uint_as_float(w[k]);
    const uint16_t b = (uint16_t)(w[k >> 1] >> (16 * (k & 1)));
    return DT == ASVD_F16 ? f16_bits_to_f32(b) : bf16_bits_to_f32(b);
}

template <int DT>
__device__ __forceinline__ void vset(uint4& r, int k, float v) {
    uint32_t* w = (uint32_t*)&r;
    if (DT == ASVD_F32) {
        w[k] = __float_as_uint(v);
    } else {
        const uint32_t b = DT == ASVD_F16 ? f32_to_f16_bits(v) : f32_to_bf16_bits(v);
        const int s = 16 * (k & 1);
        w[k >> 1] = (w[k >> 1] & ~(0xffffu << s)) | (b << s);
    }
}

// vector v of a row (elements v*VEC .. v*VEC+VEC-1): one 16-byte load when aligned, else element loads up to cols (zero beyond)
template <int DT>
__device__ __forceinline__ uint4 load_vec(const void* row, int64_t v, int64_t cols, bool vec_ok) {
    constexpr int VEC = rtn_vec<DT>::VEC;
    if (vec_ok) return ((const uint4*)row)[v];
    uint4 r = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const int64_t c = v * VEC + k;
        if (c < cols) {
            if (DT == ASVD_F32) ((uint32_t*)&r)[k] = ((const uint32_t*)row)[c];
            else ((uint16_t*)&r)[k] = ((const uint16_t*)row)[c];
        }
    }
    return r;
}

template <int DT>
__device__ __forceinline__ void store_vec(void* row, int64_t v, int64_t cols, bool vec_ok, const uint4& r) {
    constexpr int VEC = rtn_vec<DT>::VEC;
    if (vec_ok) {
        ((uint4*)row)[v] = r;
        return;
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const int64_t c = v * VEC + k;
        if (c < cols) {
            if (DT == ASVD_F32) ((uint32_t*)row)[c] = ((const uint32_t*)&r)[k];
            else ((uint16_t*)row)[c] = ((const uint16_t*)&r)[k];
        }
    }
}

template <int DT>
__device__ __forceinline__ void minmax_vec(const uint4& r, int64_t v, int64_t cols, float& mn, float& mx) {
    constexpr int VEC = rtn_vec<DT>::VEC;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        if (v * VEC + k < cols) {
            const float x = vget<DT>(r, k);
            mn = nan_min(mn, x);
            mx = nan_max(mx, x);
        }
    }
}

// quantize one vector in place; codes (if any) for its in-range elements
template <int DT>
__device__ __forceinline__ void quant_vec(uint4& r, int64_t v, int64_t cols, float scale, float zero, float maxq, uint8_t* codes_row) {
    constexpr int VEC = rtn_vec<DT>::VEC;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const float x = vget<DT>(r, k);
        float q = rintf(x / scale) + zero;
        q = (q != q) ? q : fminf(fmaxf(q, 0.0f), maxq);
        float o = scale * (q - zero);
        // the product must exist as an fp32 value before the cast: the backend otherwise folds multiply + fp32->fp16 cast into one
        // v_fma_mixlo_f16 (one rounding instead of the reference's two), whatever the contraction setting
        asm volatile("" : "+v"(o));
        vset<DT>(r, k, o);
        const int64_t c = v * VEC + k;
        if (codes_row && c < cols) codes_row[c] = (q == q) ? (uint8_t)q : (uint8_t)0;
    }
}

// min / max over the G threads of a unit (8 or 16 aligned lanes, one wave, or the whole workgroup); every thread gets the result.
// red: 2 x (RTN_THREADS / 64) floats of LDS, used only when G spans several waves
template <int G>
__device__ __forceinline__ void group_minmax(float& mn, float& mx, float* red) {
#pragma unroll
    for (int o = (G < 64 ? G : 64) / 2; o > 0; o >>= 1) {
        mn = nan_min(mn, __shfl_xor(mn, o, 64));
        mx = nan_max(mx, __shfl_xor(mx, o, 64));
    }
    if (G <= 64) return;
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[w] = mn;
        red[RTN_THREADS / 64 + w] = mx;
    }
    __syncthreads();
    mn = red[0];
    mx = red[RTN_THREADS / 64];
#pragma unroll
    for (int i = 1; i < RTN_THREADS / 64; ++i) {
        mn = nan_min(mn, red[i]);
        mx = nan_max(mx, red[RTN_THREADS / 64 + i]);
    }
}

// ---- K15: the clip search ------------------------------------------------------------------------------------------------------------

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}

// sum over the G threads of a unit in a fixed order; every thread gets the same bits.  Within 16 lanes: quad_perm [1,0,3,2], quad_perm [2,3,0,1],
// row_half_mirror, row_mirror (after each step the lanes of a quad / half / row hold one value, so the mirrors pair whole halves); across the rows
// of a wave two shuffles; across the waves of the workgroup LDS, added in wave order.  red_err: 2 x (RTN_THREADS / 64) floats, the halves used by
// alternate candidates, so that one barrier per candidate is enough
template <int G>
__device__ __forceinline__ float group_sum(float e, float* red_err, int cand) {
    e += dpp_f32<0xB1>(e);
    e += dpp_f32<0x4E>(e);
    e += dpp_f32<0x141>(e);
    if (G >= 16) e += dpp_f32<0x140>(e);
    if (G >= 64) {
        e += __shfl_xor(e, 16, 64);
        e += __shfl_xor(e, 32, 64);
    }
    if (G > 64) {
        float* r = red_err + (cand & 1) * (RTN_THREADS / 64);
        if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = e;
        __syncthreads();
        e = r[0];
#pragma unroll
        for (int i = 1; i < RTN_THREADS / 64; ++i) e += r[i];
    }
    return e;
}

// |scale1 * (clamp(rint(x / scale1) + zero1, 0, maxq) - zero1) - x|^norm, evaluated fast: r = 1 / scale1 from v_rcp_f32, the clamp taken on
// rint(x r) itself between lo = -zero1 and hi = maxq - zero1 (the same integers: all of them are below 2^24), the power as exp2(norm * log2|d|).
// x = 0 (the padding of a unit) gives exactly 0 for every finite scale1
__device__ __forceinline__ float cand_err(float x, float r, float scale1, float lo, float hi, float norm) {
    const float t = fminf(fmaxf(rintf(x * r), lo), hi);
    const float d = t * scale1 - x;
    return __builtin_amdgcn_exp2f(norm * __builtin_amdgcn_logf(fabsf(d)));
}

template <int DT>
__device__ __forceinline__ float cand_err_vec(const uint4& v, float r, float scale1, float lo, float hi, float norm) {
    constexpr int VEC = rtn_vec<DT>::VEC;
    float e = 0.0f;
#pragma unroll
    for (int k = 0; k < VEC; ++k) e += cand_err(vget<DT>(v, k), r, scale1, lo, hi, norm);
    return e;
}

// one unit quantized by G threads (tid = 0..G-1 within the group): the `cols` elements of row `row` from column c0 on (the whole row, or one
// group of it), whose scale and zero go to index sidx.  NV: vectors a thread holds on the resident path.  MSE: the clip search (K15) between the
// reduction and the final pass; ptab: its p values (LDS), red_err: see group_sum
template <int DT, int G, int NV, bool MSE>
__device__ __forceinline__ void rtn_row(const RtnTensor& T, int64_t row, int64_t c0, int64_t cols, int64_t sidx, int tid, const RtnTable& tab,
                                        float* red, const float* ptab, float* red_err) {
    constexpr int VEC = rtn_vec<DT>::VEC;
    const float maxq = tab.maxq;
    const int64_t nvec = (cols + VEC - 1) / VEC;
    const bool vec_ok = T.vec_ok != 0;
    const bool resident = G < 64 || T.resident;   // a unit of 8 or 16 lanes is a group: at most NV x G vectors
    const void* src = (const char*)T.in + (row * T.ldi + c0) * (int64_t)sizeof(typename elem<DT>::T);
    void* dst = (char*)T.out + (row * T.ldo + c0) * (int64_t)sizeof(typename elem<DT>::T);
    uint8_t* codes_row = T.codes ? T.codes + row * T.cols + c0 : nullptr;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    uint4 held[NV];
    if (resident) {
        // every load of the row is issued before the first use: the row's latency is paid once, not once per vector
        if (vec_ok) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int64_t v = tid + (int64_t)i * G;
                if (v < nvec) held[i] = ((const uint4*)src)[v];
                else if (MSE) held[i] = make_uint4(0, 0, 0, 0);   // the search adds every held element: zeros add nothing
            }
        } else {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int64_t v = tid + (int64_t)i * G;
                if (v < nvec) held[i] = load_vec<DT>(src, v, cols, false);
                else if (MSE) held[i] = make_uint4(0, 0, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int64_t v = tid + (int64_t)i * G;
            if (v < nvec) minmax_vec<DT>(held[i], v, cols, mn, mx);
        }
    } else {
        for (int64_t v = tid; v < nvec; v += G) minmax_vec<DT>(load_vec<DT>(src, v, cols, vec_ok), v, cols, mn, mx);
    }
    group_minmax<G>(mn, mx, red);
    float xmin = nan_min(mn, 0.0f), xmax = nan_max(mx, 0.0f);
    if (xmin == 0.0f && xmax == 0.0f) {
        xmin = -1.0f;
        xmax = 1.0f;
    }
    float scale = (xmax - xmin) / maxq;
    float zero = rintf(-xmin / scale);
    if (MSE) {
        // every thread of the unit runs every candidate (the reductions need them all); a unit whose base scale is 0, infinite or NaN keeps its
        // base pair, and so does every unit against a candidate whose error is NaN or infinite (err < best is false)
        const bool search = scale > 0.0f && scale < __builtin_inff();
        const float norm = tab.norm;
        const float base_scale = scale, base_zero = zero;
        float best = __builtin_inff();
        for (int c = 0; c < tab.ncand; ++c) {
            const float p = ptab[c];
            const float xmin1 = p * xmin, xmax1 = p * xmax;
            const float scale1 = (xmax1 - xmin1) / maxq;
            const float zero1 = rintf(-xmin1 / scale1);
            const float r = __builtin_amdgcn_rcpf(scale1), lo = -zero1, hi = maxq - zero1;
            float e = 0.0f;
            if (resident) {
#pragma unroll
                for (int i = 0; i < NV; ++i)
                    if ((int64_t)i * G < nvec) e += cand_err_vec<DT>(held[i], r, scale1, lo, hi, norm);
            } else {
                // two-pass rows: re-read per candidate (from cache); elements beyond cols are zero-filled by load_vec or absent (vec_ok)
                for (int64_t v = tid; v < nvec; v += G) e += cand_err_vec<DT>(load_vec<DT>(src, v, cols, vec_ok), r, scale1, lo, hi, norm);
            }
            e = group_sum<G>(e, red_err, c);
            if (search && scale1 > 0.0f && e < best) {
                best = e;
                scale = scale1;
                zero = zero1;
            }
        }
        if (!search) {
            scale = base_scale;
            zero = base_zero;
        }
    }
    if (tid == 0) {
        if (T.scale) T.scale[sidx] = scale;
        if (T.zero) T.zero[sidx] = zero;
        if (scale == 0.0f) atomicOr(T.flag, 1);
    }
    if (scale == 0.0f) {
        // the reference leaves such a tensor unchanged (Quantizer.ready()); the row is copied so that `out` holds the input, and the
        // host sees the flag.  Codes of the row are 0.
        if (resident) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int64_t v = tid + (int64_t)i * G;
                if (v < nvec) store_vec<DT>(dst, v, cols, vec_ok, held[i]);
            }
        } else {
            for (int64_t v = tid; v < nvec; v += G) store_vec<DT>(dst, v, cols, vec_ok, load_vec<DT>(src, v, cols, vec_ok));
        }
        if (codes_row)
            for (int64_t c = tid; c < cols; c += G) codes_row[c] = 0;
        return;
    }
    if (resident) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int64_t v = tid + (int64_t)i * G;
            if (v < nvec) {
                quant_vec<DT>(held[i], v, cols, scale, zero, maxq, codes_row);
                store_vec<DT>(dst, v, cols, vec_ok, held[i]);
            }
        }
    } else {
        // two-pass: every load of the first pass finished before the reduction's barrier, so `out` may alias `in`
        for (int64_t v = tid; v < nvec; v += G) {
            uint4 r = load_vec<DT>(src, v, cols, vec_ok);
            quant_vec<DT>(r, v, cols, scale, zero, maxq, codes_row);
            store_vec<DT>(dst, v, cols, vec_ok, r);
        }
    }
}

// lanes the search gives a group: those its vectors fill, 16 at the most (16 vectors of 16-bit columns or 2 x 16 of fp32 in 128, 8 or 16 in 64)
__host__ __device__ __forceinline__ int rtn_mse_sub(int dtype, int group) {
    const int nvec = group / (dtype == ASVD_F32 ? 4 : 8);
    return nvec < 16 ? nvec : 16;
}

template <bool MSE>
__global__ __launch_bounds__(RTN_THREADS) void rtn_quant_kernel(const RtnTable tab) {
    __shared__ float red[2 * (RTN_THREADS / 64)];
    __shared__ float red_err[MSE ? 2 * (RTN_THREADS / 64) : 1];
    __shared__ float ptab[MSE ? RTN_MAX_CAND : 1];
    if (MSE) {
        // p of candidate i as the reference's Python computes it: 1 - i / grid in double, then one cast to fp32
        if ((int)threadIdx.x < tab.ncand) ptab[threadIdx.x] = (float)(1.0 - (double)threadIdx.x / (double)tab.grid);
        __syncthreads();
    }
    const int64_t g = blockIdx.x;
    // the entry of this workgroup's tensor, picked with constant indices only (a run-time index into the by-value table would copy it to scratch)
    RtnTensor T = tab.t[0];
#pragma unroll
    for (int i = 1; i < RTN_MAX_BATCH; ++i)
        if (i < tab.n && g >= tab.t[i].row0) T = tab.t[i];
    if (MSE && T.group) {
        // K15 with groups: unit = row * ng + group as below, but 8 or 16 lanes per unit (rtn_mse_sub): a 16-lane DPP row holds one or two groups
        const int sub = rtn_mse_sub(T.dtype, T.group);
        const int64_t unit = ((g - T.row0) * RTN_THREADS + threadIdx.x) / sub;
        const int64_t row = unit / T.ng, c0 = (unit - row * T.ng) * T.group;
        const int64_t cols = T.cols - c0 < T.group ? T.cols - c0 : (int64_t)T.group;
        if (row >= T.rows) return;
        if (sub == 16) {
            const int lane = threadIdx.x & 15;
            switch (T.dtype) {
                case ASVD_F32: rtn_row<ASVD_F32, 16, 2, MSE>(T, row, c0, cols, unit, lane, tab, red, ptab, red_err); break;
                case ASVD_F16: rtn_row<ASVD_F16, 16, 1, MSE>(T, row, c0, cols, unit, lane, tab, red, ptab, red_err); break;
                default: rtn_row<ASVD_BF16, 16, 1, MSE>(T, row, c0, cols, unit, lane, tab, red, ptab, red_err); break;
            }
        } else {   // groups of 8 vectors: 64 columns of a 16-bit type
            const int lane = threadIdx.x & 7;
            if (T.dtype == ASVD_F16) rtn_row<ASVD_F16, 8, 1, MSE>(T, row, c0, cols, unit, lane, tab, red, ptab, red_err);
            else rtn_row<ASVD_BF16, 8, 1, MSE>(T, row, c0, cols, unit, lane, tab, red, ptab, red_err);
        }
        return;
    }
    if (T.per_wave) {  // rows of up to 64 x RTN_NV vectors: one wave per row, RTN_THREADS / 64 rows per workgroup, no barrier
        const int64_t unit = (g - T.row0) * (RTN_THREADS / 64) + (threadIdx.x >> 6);
        // K14: unit = row * ng + group; the group's columns start at group * G and the last group of a row holds what is left
        int64_t row = unit, c0 = 0, cols = T.cols;
        if (T.group) {
            row = unit / T.ng;
            c0 = (unit - row * T.ng) * T.group;
            cols = cols - c0 < T.group ? cols - c0 : (int64_t)T.group;
        }
        if (row >= T.rows) return;
        const int lane = threadIdx.x & 63;
        switch (T.dtype) {
            case ASVD_F32: rtn_row<ASVD_F32, 64, RTN_NV, MSE>(T, row, c0, cols, unit, lane, tab, red, ptab, red_err); break;
            case ASVD_F16: rtn_row<ASVD_F16, 64, RTN_NV, MSE>(T, row, c0, cols, unit, lane, tab, red, ptab, red_err); break;
            default: rtn_row<ASVD_BF16, 64, RTN_NV, MSE>(T, row, c0, cols, unit, lane, tab, red, ptab, red_err); break;
        }
        return;
    }
    const int64_t row = g - T.row0;
    switch (T.dtype) {
        case ASVD_F32: rtn_row<ASVD_F32, RTN_THREADS, RTN_NV, MSE>(T, row, 0, T.cols, row, threadIdx.x, tab, red, ptab, red_err); break;
        case ASVD_F16: rtn_row<ASVD_F16, RTN_THREADS, RTN_NV, MSE>(T, row, 0, T.cols, row, threadIdx.x, tab, red, ptab, red_err); break;
        default: rtn_row<ASVD_BF16, RTN_THREADS, RTN_NV, MSE>(T, row, 0, T.cols, row, threadIdx.x, tab, red, ptab, red_err); break;
    }
}

bool rtn_args_ok(const void* w, int dtype, int64_t rows, int64_t cols, int64_t ldw, const void* out, int64_t ldo) {
    return w && out && rows >= 1 && cols >= 1 && ldw >= cols && ldo >= cols && dtype_ok(dtype);
}

struct RtnMse {   // K15: validated search parameters
    float norm;
    int grid, ncand;
};

// group: 0 (one scale and zero per row) or 64 / 128 (K14: per group of that many columns); mse: NULL, or the clip search (K15)
int rtn_launch_batched(int batch, const void* const* w_host, const int* dtype_host, const int64_t* rows_host, const int64_t* cols_host,
                       const int64_t* ldw_host, int bits, void* const* out_host, const int64_t* ldo_host, float* const* scale_host,
                       float* const* zero_host, void* const* codes_host, int group, int* flags, void* stream, const RtnMse* mse = nullptr) {
    if (batch < 1 || !w_host || !dtype_host || !rows_host || !cols_host || !ldw_host || !out_host || !ldo_host || !flags) return ASVD_E_BADARG;
    if (bits < 1 || bits > 8) return ASVD_E_BADARG;
    for (int b = 0; b < batch; ++b)
        if (!rtn_args_ok(w_host[b], dtype_host[b], rows_host[b], cols_host[b], ldw_host[b], out_host[b], ldo_host[b])) return ASVD_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    for (int b0 = 0; b0 < batch; b0 += RTN_MAX_BATCH) {
        RtnTable tab;
        memset(&tab, 0, sizeof(tab));
        tab.n = (batch - b0 < RTN_MAX_BATCH) ? batch - b0 : RTN_MAX_BATCH;
        tab.maxq = (float)((1 << bits) - 1);
        if (mse) {
            tab.norm = mse->norm;
            tab.grid = mse->grid;
            tab.ncand = mse->ncand;
        }
        int64_t row0 = 0;
        for (int i = 0; i < tab.n; ++i) {
            const int b = b0 + i;
            RtnTensor& T = tab.t[i];
            const int dt = dtype_host[b];
            const int64_t es = (int64_t)dtype_size(dt), vec = 16 / es;
            T.in = w_host[b];
            T.out = out_host[b];
            T.scale = scale_host ? scale_host[b] : nullptr;
            T.zero = zero_host ? zero_host[b] : nullptr;
            T.codes = codes_host ? (uint8_t*)codes_host[b] : nullptr;
            T.flag = flags + b;
            T.row0 = row0;
            T.rows = rows_host[b];
            T.cols = cols_host[b];
            T.ldi = ldw_host[b];
            T.ldo = ldo_host[b];
            T.dtype = dt;
            T.vec_ok = ((uintptr_t)T.in % 16 == 0) && ((uintptr_t)T.out % 16 == 0) && ((T.ldi * es) % 16 == 0) && ((T.ldo * es) % 16 == 0) &&
                       (T.cols % vec == 0);
            T.group = group;
            T.ng = group ? ceil_div64(T.cols, group) : 1;   // a group starts 16-byte aligned in an aligned row: vec_ok is the row's
            const int64_t nvec = ceil_div64(group ? (int64_t)group : T.cols, vec);
            T.per_wave = nvec <= (int64_t)RTN_NV * 64;      // a group is at most 32 vectors: always
            T.resident = nvec <= (int64_t)RTN_NV * (T.per_wave ? 64 : RTN_THREADS);
            if (group && T.rows > 0x7fffffffffff / T.ng) return ASVD_E_BADARG;
            const int64_t units_per_wg = (mse && group) ? RTN_THREADS / rtn_mse_sub(dt, group) : RTN_THREADS / 64;
            row0 += T.per_wave ? ceil_div64(T.rows * T.ng, units_per_wg) : T.rows;
        }
        if (row0 > 0x7fffffff) return ASVD_E_BADARG;
        if (mse) rtn_quant_kernel<true><<<(unsigned)row0, RTN_THREADS, 0, st>>>(tab);
        else rtn_quant_kernel<false><<<(unsigned)row0, RTN_THREADS, 0, st>>>(tab);
        ASVD_HIP_CHECK(hipGetLastError());
    }
    return ASVD_OK;
}

}  // namespace

extern "C" {

int asvd_rtn_quant_batched(int batch, const void* const* w_host, const int* dtype_host, const int64_t* rows_host, const int64_t* cols_host,
                           const int64_t* ldw_host, int bits, void* const* out_host, const int64_t* ldo_host, float* const* scale_host,
                           float* const* zero_host, void* const* codes_host, int* flags, void* stream) {
    return rtn_launch_batched(batch, w_host, dtype_host, rows_host, cols_host, ldw_host, bits, out_host, ldo_host, scale_host, zero_host, codes_host,
                              0, flags, stream);
}

int asvd_rtn_quant_grouped_batched(int batch, const void* const* w_host, const int* dtype_host, const int64_t* rows_host, const int64_t* cols_host,
                                   const int64_t* ldw_host, int bits, void* const* out_host, const int64_t* ldo_host, float* const* scale_host,
                                   float* const* zero_host, void* const* codes_host, int* flags, void* stream, int64_t group) {
    if (group != 64 && group != 128) return ASVD_E_BADARG;
    return rtn_launch_batched(batch, w_host, dtype_host, rows_host, cols_host, ldw_host, bits, out_host, ldo_host, scale_host, zero_host, codes_host,
                              (int)group, flags, stream);
}

int asvd_rtn_quant_mse_batched(int batch, const void* const* w_host, const int* dtype_host, const int64_t* rows_host, const int64_t* cols_host,
                               const int64_t* ldw_host, int bits, void* const* out_host, const int64_t* ldo_host, float* const* scale_host,
                               float* const* zero_host, void* const* codes_host, int* flags, void* stream, int64_t group, float norm, int grid,
                               float maxshrink) {
    if (group != 0 && group != 64 && group != 128) return ASVD_E_BADARG;
    if (!(norm > 0.0f) || !std::isfinite(norm) || grid < 1 || !(maxshrink > 0.0f) || !(maxshrink <= 1.0f)) return ASVD_E_BADARG;
    // the candidate count is Python's int(maxshrink * grid) in double.  maxshrink arrives as a float: the double taken is the shortest decimal
    // that reads back as that float (0.7f counts as 0.7, 70 candidates of a grid of 100, not as 0.699999988..., 69)
    double shrink = (double)maxshrink;
    for (int prec = 1; prec <= 9; ++prec) {
        char buf[32];
        snprintf(buf, sizeof(buf), "%.*g", prec, (double)maxshrink);
        const double d = strtod(buf, nullptr);
        if ((float)d == maxshrink) {
            shrink = d;
            break;
        }
    }
    const double cand = shrink * (double)grid;
    if (!(cand >= 1.0) || cand >= (double)(RTN_MAX_CAND + 1)) return ASVD_E_BADARG;
    const RtnMse mse = {norm, grid, (int)cand};
    return rtn_launch_batched(batch, w_host, dtype_host, rows_host, cols_host, ldw_host, bits, out_host, ldo_host, scale_host, zero_host, codes_host,
                              (int)group, flags, stream, &mse);
}

int asvd_rtn_quant_grouped(const void* w, int dtype, int64_t rows, int64_t cols, int64_t ldw, int bits, void* out, int64_t ldo, float* scale,
                           float* zero, void* codes, int* flag, void* stream, int64_t group) {
    if (!rtn_args_ok(w, dtype, rows, cols, ldw, out, ldo) || !flag || bits < 1 || bits > 8) return ASVD_E_BADARG;
    return asvd_rtn_quant_grouped_batched(1, &w, &dtype, &rows, &cols, &ldw, bits, &out, &ldo, &scale, &zero, &codes, flag, stream, group);
}

int asvd_rtn_quant(const void* w, int dtype, int64_t rows, int64_t cols, int64_t ldw, int bits, void* out, int64_t ldo, float* scale, float* zero,
                   void* codes, int* flag, void* stream) {
    if (!rtn_args_ok(w, dtype, rows, cols, ldw, out, ldo) || !flag || bits < 1 || bits > 8) return ASVD_E_BADARG;
    return asvd_rtn_quant_batched(1, &w, &dtype, &rows, &cols, &ldw, bits, &out, &ldo, &scale, &zero, &codes, flag, stream);
}

}  // extern "C"
