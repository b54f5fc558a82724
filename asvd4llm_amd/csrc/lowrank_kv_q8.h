// lowrank_kv_q8.h — the int8 form of the low-rank KV cache (K21): the one definition the quantiser (lowrank_kv_q8.hip) and the
// dequantise-in-registers loaders of K20 (lowrank_kv.hip) share.
//
// A cache row x[0 .. r) (fp16, r a multiple of 16) is cut into groups of 32 consecutive columns; when r % 32 == 16 the last group has 16.
// Per group: amax = max |x|, s = amax / 127 (IEEE fp32 division), code = clamp(rintf(float(x) / s), -127, 127) as int8.  amax == 0 gives
// s = 0 and codes 0; a NaN or Inf in the group gives s = NaN (0x7fc00000) and codes 0, so the whole group reads back as NaN.
// Read back: d = fp16_rne(float(code) * s), one fp32 product and one rounding, defined for every int8 code.
// The bf16 kernels (K22) use bf16_rne(d): the SAME format and the same d, rounded once more (a double rounding by design: it is the value
// torch's dequantise-then-.bfloat16() gives, so kernel and torch path read one cache).
#pragma once
#include "common.h"

constexpr int KV_Q8_GROUP = 32;   // columns per scale

static inline int64_t kv_q8_groups(int64_t r) { return (r + KV_Q8_GROUP - 1) / KV_Q8_GROUP; }

__device__ __forceinline__ _Float16 kv_q8_dequant(int code, float s) {
#pragma clang fp contract(off)
    const float p = (float)code * s;
    return (_Float16)p;
}

// 8 codes (byte u of the pair is column u) of one group -> 8 fp16 values
__device__ __forceinline__ f16x8 kv_q8_dequant8(uint2 c, float s) {
    f16x8 d;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        d[u] = kv_q8_dequant((int)(int8_t)(c.x >> (8 * u)), s);
        d[4 + u] = kv_q8_dequant((int)(int8_t)(c.y >> (8 * u)), s);
    }
    return d;
}

// K22: the bits of bf16_rne(d)
__device__ __forceinline__ uint16_t kv_q8_dequant_bf16(int code, float s) { return f32_to_bf16_bits((float)kv_q8_dequant(code, s)); }

__device__ __forceinline__ f16x8 kv_q8_dequant8_bf16(uint2 c, float s) {   // f16x8 as the container of 8 bf16 values
    f16x8 d;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        d[u] = __builtin_bit_cast(_Float16, kv_q8_dequant_bf16((int)(int8_t)(c.x >> (8 * u)), s));
        d[4 + u] = __builtin_bit_cast(_Float16, kv_q8_dequant_bf16((int)(int8_t)(c.y >> (8 * u)), s));
    }
    return d;
}
