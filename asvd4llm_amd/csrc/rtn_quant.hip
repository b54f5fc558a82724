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
#include "common.h"
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
};

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

// min / max over the G threads of a row (one wave, or the whole workgroup); every thread gets the result.  red: 2 x (RTN_THREADS / 64)
// floats of LDS, used only when G spans several waves
template <int G>
__device__ __forceinline__ void group_minmax(float& mn, float& mx, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = nan_min(mn, __shfl_xor(mn, o, 64));
        mx = nan_max(mx, __shfl_xor(mx, o, 64));
    }
    if (G == 64) return;
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

// one unit quantized by G threads (tid = 0..G-1 within the group): the `cols` elements of row `row` from column c0 on (the whole row, or one
// group of it), whose scale and zero go to index sidx
template <int DT, int G>
__device__ __forceinline__ void rtn_row(const RtnTensor& T, int64_t row, int64_t c0, int64_t cols, int64_t sidx, int tid, float maxq, float* red) {
    constexpr int VEC = rtn_vec<DT>::VEC;
    const int64_t nvec = (cols + VEC - 1) / VEC;
    const bool vec_ok = T.vec_ok != 0;
    const void* src = (const char*)T.in + (row * T.ldi + c0) * (int64_t)sizeof(typename elem<DT>::T);
    void* dst = (char*)T.out + (row * T.ldo + c0) * (int64_t)sizeof(typename elem<DT>::T);
    uint8_t* codes_row = T.codes ? T.codes + row * T.cols + c0 : nullptr;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    uint4 held[RTN_NV];
    if (T.resident) {
        // every load of the row is issued before the first use: the row's latency is paid once, not once per vector
        if (vec_ok) {
#pragma unroll
            for (int i = 0; i < RTN_NV; ++i) {
                const int64_t v = tid + (int64_t)i * G;
                if (v < nvec) held[i] = ((const uint4*)src)[v];
            }
        } else {
#pragma unroll
            for (int i = 0; i < RTN_NV; ++i) {
                const int64_t v = tid + (int64_t)i * G;
                if (v < nvec) held[i] = load_vec<DT>(src, v, cols, false);
            }
        }
#pragma unroll
        for (int i = 0; i < RTN_NV; ++i) {
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
    const float scale = (xmax - xmin) / maxq;
    const float zero = rintf(-xmin / scale);
    if (tid == 0) {
        if (T.scale) T.scale[sidx] = scale;
        if (T.zero) T.zero[sidx] = zero;
        if (scale == 0.0f) atomicOr(T.flag, 1);
    }
    if (scale == 0.0f) {
        // the reference leaves such a tensor unchanged (Quantizer.ready()); the row is copied so that `out` holds the input, and the
        // host sees the flag.  Codes of the row are 0.
        if (T.resident) {
#pragma unroll
            for (int i = 0; i < RTN_NV; ++i) {
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
    if (T.resident) {
#pragma unroll
        for (int i = 0; i < RTN_NV; ++i) {
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

__global__ __launch_bounds__(RTN_THREADS) void rtn_quant_kernel(const RtnTable tab) {
    __shared__ float red[2 * (RTN_THREADS / 64)];
    const int64_t g = blockIdx.x;
    // the entry of this workgroup's tensor, picked with constant indices only (a run-time index into the by-value table would copy it to scratch)
    RtnTensor T = tab.t[0];
#pragma unroll
    for (int i = 1; i < RTN_MAX_BATCH; ++i)
        if (i < tab.n && g >= tab.t[i].row0) T = tab.t[i];
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
            case ASVD_F32: rtn_row<ASVD_F32, 64>(T, row, c0, cols, unit, lane, tab.maxq, red); break;
            case ASVD_F16: rtn_row<ASVD_F16, 64>(T, row, c0, cols, unit, lane, tab.maxq, red); break;
            default: rtn_row<ASVD_BF16, 64>(T, row, c0, cols, unit, lane, tab.maxq, red); break;
        }
        return;
    }
    const int64_t row = g - T.row0;
    switch (T.dtype) {
        case ASVD_F32: rtn_row<ASVD_F32, RTN_THREADS>(T, row, 0, T.cols, row, threadIdx.x, tab.maxq, red); break;
        case ASVD_F16: rtn_row<ASVD_F16, RTN_THREADS>(T, row, 0, T.cols, row, threadIdx.x, tab.maxq, red); break;
        default: rtn_row<ASVD_BF16, RTN_THREADS>(T, row, 0, T.cols, row, threadIdx.x, tab.maxq, red); break;
    }
}

bool rtn_args_ok(const void* w, int dtype, int64_t rows, int64_t cols, int64_t ldw, const void* out, int64_t ldo) {
    return w && out && rows >= 1 && cols >= 1 && ldw >= cols && ldo >= cols && dtype_ok(dtype);
}

// group: 0 (one scale and zero per row) or 64 / 128 (K14: per group of that many columns)
int rtn_launch_batched(int batch, const void* const* w_host, const int* dtype_host, const int64_t* rows_host, const int64_t* cols_host,
                       const int64_t* ldw_host, int bits, void* const* out_host, const int64_t* ldo_host, float* const* scale_host,
                       float* const* zero_host, void* const* codes_host, int group, int* flags, void* stream) {
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
            row0 += T.per_wave ? ceil_div64(T.rows * T.ng, RTN_THREADS / 64) : T.rows;
        }
        if (row0 > 0x7fffffff) return ASVD_E_BADARG;
        rtn_quant_kernel<<<(unsigned)row0, RTN_THREADS, 0, st>>>(tab);
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
