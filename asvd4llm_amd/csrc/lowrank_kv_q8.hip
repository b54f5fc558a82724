// lowrank_kv_q8.hip — K21: quantise new rows of the low-rank KV cache to int8 codes and group scales on append.
//
// The format is lowrank_kv_q8.h's: groups of 32 latent columns (a 16-wide tail when r % 32 == 16), s = amax / 127 in fp32,
// code = clamp(rintf(x / s), -127, 127).  Every step is its own fp32 rounding (IEEE division, rintf = round half to even, no contraction),
// so the codes and scales are those of the torch definition (ops.lowrank_kv_quant_torch) bit for bit.
//
// One launch for all B * n new rows.  A group is 64 bytes of fp16: FOUR lanes take it, one 16-byte load each (two lanes of a quad idle on
// the 16-wide tail), reduce |x| and the non-finite flag with two shuffles inside the quad, and store 8 codes each as one 8-byte vector store;
// the quad's first lane stores the scale.  Every row is padded to 4 * ng lanes so that quads never straddle rows or waves.  No LDS, no atomics,
// no host sync; the only addresses written are the r code bytes and the ng scales of the B * n destination rows (strided: a slice
// [:, t0 : t0 + n] of the cache).
#include "lowrank_kv_q8.h"

#pragma clang fp contract(off)

namespace {

constexpr int KVQ_THREADS = 256;
constexpr int KVQ_MAX_RANK = 16384;   // K20's largest rank

__global__ __launch_bounds__(KVQ_THREADS) void kv_quant_kernel(const uint16_t* __restrict__ x, int64_t xrs, int64_t xbs, int8_t* __restrict__ codes,
                                                               int64_t crs, int64_t cbs, float* __restrict__ scales, int64_t srs, int64_t sbs,
                                                               int64_t total, int n, int r, int ng) {
    const int64_t gid = (int64_t)blockIdx.x * KVQ_THREADS + threadIdx.x;
    if (gid >= total) return;   // total is a multiple of 4: whole quads leave together
    const int upr = 4 * ng;     // lanes per row
    const int64_t row = gid / upr;
    const int v = (int)(gid - row * upr), c0 = 8 * v;
    const int64_t b = row / n, t = row - b * n;
    const bool active = c0 < r;   // false for the two idle lanes of a 16-wide tail group; they still take part in the shuffles
    uint4 raw = make_uint4(0u, 0u, 0u, 0u);
    if (active) raw = *(const uint4*)(x + b * xbs + t * xrs + c0);
    const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
    float xv[8];
    float amax = 0.f;
    int bad = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const uint16_t h = (uint16_t)(w[u >> 1] >> (16 * (u & 1)));
        bad |= (h & 0x7c00u) == 0x7c00u;   // Inf or NaN; fmaxf would drop a NaN
        xv[u] = f16_bits_to_f32(h);
        amax = fmaxf(amax, fabsf(xv[u]));
    }
#pragma unroll
    for (int o = 1; o < 4; o <<= 1) {
        amax = fmaxf(amax, __shfl_xor(amax, o, 64));
        bad |= __shfl_xor(bad, o, 64);
    }
    const float s = bad ? __uint_as_float(0x7fc00000u) : amax / 127.0f;
    if (!active) return;
    const bool zero = bad || amax == 0.f;
    const float sd = zero ? 1.f : s;   // a group of zeros or with a non-finite value: all codes 0, nothing is divided by 0 or NaN
    uint32_t pk[2] = {0u, 0u};
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const float qf = fminf(fmaxf(rintf(xv[u] / sd), -127.f), 127.f);
        const int code = zero ? 0 : (int)qf;
        pk[u >> 2] |= (uint32_t)(code & 0xff) << (8 * (u & 3));
    }
    *(uint2*)(codes + b * cbs + t * crs + c0) = make_uint2(pk[0], pk[1]);
    if ((v & 3) == 0) scales[b * sbs + t * srs + (v >> 2)] = s;
}

inline bool mis16(const void* p) { return ((uintptr_t)p & 15) != 0; }

}  // namespace

extern "C" int asvd_lowrank_kv_quant(const void* x, int64_t x_row_stride, int64_t x_batch_stride, void* codes, int64_t c_row_stride,
                                     int64_t c_batch_stride, void* scales, int64_t s_row_stride, int64_t s_batch_stride, int dtype, int64_t B,
                                     int64_t n, int64_t r, void* stream) {
    if (!x || !codes || !scales) return ASVD_E_BADARG;
    if (dtype != ASVD_F16) return ASVD_E_BADARG;
    if (B < 1 || B > (1 << 20) || n < 1 || n > (1 << 22)) return ASVD_E_BADARG;
    if (r < 16 || r % 16 || r > KVQ_MAX_RANK) return ASVD_E_BADARG;
    const int64_t ng = kv_q8_groups(r);
    if (mis16(x) || mis16(codes) || ((uintptr_t)scales & 3)) return ASVD_E_BADARG;
    if (x_row_stride < r || x_row_stride % 8 || x_batch_stride % 8 || x_batch_stride < 0 || (B > 1 && x_batch_stride < n * x_row_stride)) return ASVD_E_BADARG;
    if (c_row_stride < r || c_row_stride % 16 || c_batch_stride % 16 || c_batch_stride < 0 || (B > 1 && c_batch_stride < n * c_row_stride)) return ASVD_E_BADARG;
    if (s_row_stride < ng || s_batch_stride < 0 || (B > 1 && s_batch_stride < n * s_row_stride)) return ASVD_E_BADARG;
    const int64_t total = B * n * 4 * ng;
    if (ceil_div64(total, KVQ_THREADS) > 0x7fffffff) return ASVD_E_BADARG;
    hipLaunchKernelGGL(kv_quant_kernel, dim3((unsigned)ceil_div64(total, KVQ_THREADS)), dim3(KVQ_THREADS), 0, (hipStream_t)stream, (const uint16_t*)x,
                       x_row_stride, x_batch_stride, (int8_t*)codes, c_row_stride, c_batch_stride, (float*)scales, s_row_stride, s_batch_stride, total,
                       (int)n, (int)r, (int)ng);
    ASVD_HIP_CHECK(hipGetLastError());
    return ASVD_OK;
}
