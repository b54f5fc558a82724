// lowrank_kv.hip — K20: one decode step of attention on a LOW-RANK KV cache (ASVD k_proj / v_proj = ALinear(BLinear(x))).
//
// The cache holds the r-wide BLinear outputs C_k [B, Tmax, r_k] and C_v [B, Tmax, r_v] (fp16) instead of K and V.  With
// K_h = C_k A_k[h]^T and V_h = C_v A_v[h]^T (A_* = the ALinear weights, [H_kv * D, r] row-major):
//
//   values            softmax(s_h) V_h = (p_h C_v) A_v[h]^T : the weighted sum runs in the r_v-wide latent space, A_v is applied to ONE
//                     r_v vector per head afterwards, b_v is added once (sum p = 1).
//   keys, no rotation q_h . K_h[t] = (A_k[h]^T q_h) . C_k[t] : scores are a [H, r_k] x [r_k, T] product that reads the cache once.
//   keys under RoPE   the rotation depends on t: the kernel rebuilds K_h one 32-token tile at a time on the matrix pipe, rotates the
//                     fp32 tile with the caller's cos / sin rows and dots it with the (already rotated) q_h.  K is never written.
//
// Five ordinary launches on the caller's stream, in this order; no grid barrier, no atomics, lengths read on the device:
//   a  kv_qtilde_kernel        q~[b, h, :] = fp16(A_k[kv(h)]^T q[b, h, :])                         (mode NONE only)
//   b  kv_scores_none_kernel   S[b, h, t] = scale * q~[b, h, :] . C_k[b, t, :]   for t < len[b]    (fp32, [B, H, Tld])
//      kv_scores_half_kernel   S[b, h, t] = scale * q[b, h, :] . rot_t(C_k[b, t, :] A_k[kv(h)]^T)
//   c  kv_pv_kernel            per split of the tokens: m = max S, p = fp16(exp(S - m)), l = sum p, O~[h, :] = p C_v  (fp32 partials)
//   d  kv_combine_kernel       merge the splits in index order, out[b, h, :] = fp16(A_v[kv(h)] O~[b, h, :] / l + b_v)
//
// Every matrix product is v_mfma_f32_32x32x16_f16 fed straight from global memory (lane (i, g) holds row / column i, reduction
// indices 8g .. 8g+7).  An output element of that instruction depends on its own operand row and column only, so rows that stand for
// padded heads, padded rank columns or tokens >= len[b] are loaded from a clamped, valid address and simply never stored; where a
// masked TOKEN is a reduction index (stage c) its p is set to 0 by a select and its cache value is replaced by 0, never multiplied.
// Nothing at positions >= len[b] of a cache, the unwritten tail of S included, can reach an output; a non-finite value in one
// sequence's cache or query stays in that sequence (no reduction crosses b).  Two calls give the same bits: no order depends on timing.
//
// K21: the cache may hold int8 codes and one fp32 scale per token and 32 rank columns instead (the format of lowrank_kv_q8.h).  Stages b and c
// are templated on that; the two forms differ ONLY in how a lane obtains its cache operand (KvTok, KvCol below): the int8 form loads 8 codes
// (stage b: 8 columns of one token, one 8-byte load and one scale; stage c: 8 tokens of one column, a byte and a scale each) and
// dequantises them in registers, d = fp16(float(code) * s).  The fp16 values then feed the same MFMA in the same order, so an int8 call
// returns the bits of the fp16 call on the dequantised cache.  Masked tokens load code AND scale from the clamped address and are replaced
// by 0 with the same select.  Stages a and d, the plan and the workspace do not depend on the cache format.
//
// K22: every stage is templated on the 16-bit element type ADT (ASVD_F16 or ASVD_BF16: the type of q, A_k, A_v, the biases, the output and of an
// unquantised cache), reached through the asvd_lowrank_kv_*_a16 entries.  The bf16 form is the same text with bf16 loads, one RNE rounding to
// bf16 wherever the fp16 form rounds to fp16 (q~, p, out) and v_mfma_f32_32x32x16_bf16, whose operand and accumulator layout is the fp16
// instruction's; plan, workspace, geometry, masking and the order of every sum are shared.  On an int8 cache the bf16 form uses
// bf16_rne(fp16_rne(float(code) * s)): K21's value, rounded once more (what cache.read(..., torch.bfloat16) hands the torch path).
#include "lowrank_kv_q8.h"

namespace {

constexpr int KV_TOK_TILE = 128;   // tokens per workgroup in stage b: one 32-token MFMA tile per wave
constexpr int KV_MIN_SPLIT = 64;   // shortest split of stage c (tokens), a multiple of 16
constexpr int KV_MAX_SPLITS = 16;  // most splits: bounds the fp32 partials (ns * H * r_v * 4 bytes per sequence)
constexpr int KV_CUS = 256;        // compute units of the gfx950 parts (MI350X / MI355X): the split count aims at one workgroup per CU
constexpr int KV_MAX_RANK = 16384; // stage d keeps one r_v-wide fp32 vector in LDS (64 KiB)

struct KvPlan {
    int64_t hpad, tld, split_len, n_splits;
    size_t off_qt, off_s, off_ml, off_o, total;
};

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// the geometry and the workspace layout: a function of (B, H, Tmax, ranks) and of the constant CU count only
KvPlan kv_plan(int64_t B, int64_t H, int64_t Tmax, int64_t r_k, int64_t r_v) {
    KvPlan p;
    p.hpad = round_up64(H, 32);
    p.tld = round_up64(Tmax, 16);
    const int64_t wgs = B * (p.hpad / 32);
    int64_t want = ceil_div64(KV_CUS, wgs);
    if (want > KV_MAX_SPLITS) want = KV_MAX_SPLITS;
    int64_t L = round_up64(ceil_div64(Tmax, want), 16);
    if (L < KV_MIN_SPLIT) L = KV_MIN_SPLIT;
    p.split_len = L;
    p.n_splits = ceil_div64(Tmax, L);
    p.off_qt = 0;
    p.off_s = up256((size_t)(B * p.hpad * r_k) * 2);
    p.off_ml = p.off_s + up256((size_t)(B * H * p.tld) * 4);
    p.off_o = p.off_ml + up256((size_t)(B * p.n_splits * p.hpad * 2) * 4);
    p.total = p.off_o + up256((size_t)(B * p.n_splits * p.hpad * r_v) * 4);
    return p;
}

__device__ __forceinline__ int kv_len(const int* __restrict__ lens, int b, int Tmax) { return min(max(lens[b], 0), Tmax); }
// accumulator register q of lane half g -> row of the 32 x 32 tile (the column is lane & 31)
__device__ __forceinline__ int acc_row(int q, int g) { return (q & 3) + 8 * (q >> 2) + 4 * g; }

// ---- ADT, the 16-bit element type: the two forms differ in these three helpers (element load, RNE rounding, matrix instruction) only ----
typedef __bf16 kv_bf16x8 __attribute__((ext_vector_type(8)));
template <int ADT>
__device__ __forceinline__ float kv_to_f32(uint16_t b) {
    return ADT == ASVD_BF16 ? bf16_bits_to_f32(b) : f16_bits_to_f32(b);
}
template <int ADT>
__device__ __forceinline__ uint16_t kv_from_f32(float v) {
    return ADT == ASVD_BF16 ? f32_to_bf16_bits(v) : f32_to_f16_bits(v);
}
// a, b: 8 values of type ADT each; f16x8 is their container in both forms
template <int ADT>
__device__ __forceinline__ f32x16 kv_mfma(f16x8 a, f16x8 b, f32x16 acc) {
    if constexpr (ADT == ASVD_BF16)
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(kv_bf16x8, a), __builtin_bit_cast(kv_bf16x8, b), acc, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
}

// ---- a: q~ = ADT(A_k[kv(h)]^T q) -------------------------------------------------------------------------------------------------
template <int ADT>
__global__ __launch_bounds__(256) void kv_qtilde_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ Ak, uint16_t* __restrict__ qt,
                                                        int H, int group, int D, int r_k, int hpad) {
    __shared__ float qs[128];
    const int b = blockIdx.x / H, h = blockIdx.x % H, kvh = h / group, tid = threadIdx.x;
    if (tid < D) qs[tid] = kv_to_f32<ADT>(q[((int64_t)b * H + h) * D + tid]);
    __syncthreads();
    const int j = blockIdx.y * 256 + tid;
    if (j >= r_k) return;
    const uint16_t* a = Ak + (int64_t)kvh * D * r_k + j;
    float acc = 0.f;
    for (int d = 0; d < D; ++d) acc += kv_to_f32<ADT>(a[(int64_t)d * r_k]) * qs[d];
    qt[((int64_t)b * hpad + h) * r_k + j] = kv_from_f32<ADT>(acc);
}

// ---- how a lane obtains its cache operand: Q8 = false reads ADT values, Q8 = true int8 codes and their group scales (K21) --------------
// stage b: the 8 rank columns 16 k + 8 g .. + 7 of token t; they lie in ONE 32-column group, k >> 1
template <int ADT, bool Q8> struct KvTok;
template <int ADT> struct KvTok<ADT, false> {
    const uint4* p;
    __device__ __forceinline__ KvTok(const void* c, int64_t rs, int64_t bs, const float*, int64_t, int64_t, int b, int t, int g)
        : p((const uint4*)((const uint16_t*)c + (int64_t)b * bs + (int64_t)t * rs + 8 * g)) {}
    __device__ __forceinline__ f16x8 operator()(int k) const { return __builtin_bit_cast(f16x8, p[2 * k]); }
};
template <int ADT> struct KvTok<ADT, true> {
    const uint2* p;
    const float* s;
    __device__ __forceinline__ KvTok(const void* c, int64_t rs, int64_t bs, const float* sc, int64_t srs, int64_t sbs, int b, int t, int g)
        : p((const uint2*)((const int8_t*)c + (int64_t)b * bs + (int64_t)t * rs + 8 * g)), s(sc + (int64_t)b * sbs + (int64_t)t * srs) {}
    __device__ __forceinline__ f16x8 operator()(int k) const {
        if constexpr (ADT == ASVD_BF16) return kv_q8_dequant8_bf16(p[2 * k], s[k >> 1]);
        else return kv_q8_dequant8(p[2 * k], s[k >> 1]);
    }
};
// stage c: rank column j of any token t (the bits of the ADT value)
template <int ADT, bool Q8> struct KvCol;
template <int ADT> struct KvCol<ADT, false> {
    const uint16_t* p;
    int64_t rs;
    __device__ __forceinline__ KvCol(const void* c, int64_t rs_, int64_t bs, const float*, int64_t, int64_t, int b, int j)
        : p((const uint16_t*)c + (int64_t)b * bs + j), rs(rs_) {}
    __device__ __forceinline__ uint16_t operator()(int t) const { return p[(int64_t)t * rs]; }
};
template <int ADT> struct KvCol<ADT, true> {
    const int8_t* p;
    const float* s;
    int64_t rs, srs;
    __device__ __forceinline__ KvCol(const void* c, int64_t rs_, int64_t bs, const float* sc, int64_t srs_, int64_t sbs, int b, int j)
        : p((const int8_t*)c + (int64_t)b * bs + j), s(sc + (int64_t)b * sbs + j / KV_Q8_GROUP), rs(rs_), srs(srs_) {}
    __device__ __forceinline__ uint16_t operator()(int t) const {
        if constexpr (ADT == ASVD_BF16) return kv_q8_dequant_bf16((int)p[(int64_t)t * rs], s[(int64_t)t * srs]);
        else return __builtin_bit_cast(uint16_t, kv_q8_dequant((int)p[(int64_t)t * rs], s[(int64_t)t * srs]));
    }
};

// ---- b, no rotation: S = scale * q~ C_k^T, heads in the accumulator registers, tokens on the lanes (coalesced stores) -----------------
template <int ADT, bool Q8>
__global__ __launch_bounds__(256) void kv_scores_none_kernel(const uint16_t* __restrict__ qt, const void* __restrict__ ck, int64_t rs, int64_t bs,
                                                             const float* __restrict__ sk, int64_t srs, int64_t sbs, const int* __restrict__ lens,
                                                             float* __restrict__ S, float scale, int H, int r_k, int Tmax, int hpad, int tld) {
    const int b = blockIdx.x, len = kv_len(lens, b, Tmax);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, i = lane & 31, g = lane >> 5;
    const int t0 = blockIdx.y * KV_TOK_TILE + wave * 32, h0 = blockIdx.z * 32;
    if (t0 >= len) return;
    const uint4* qp = (const uint4*)(qt + ((int64_t)b * hpad + min(h0 + i, H - 1)) * r_k + 8 * g);
    const KvTok<ADT, Q8> cp(ck, rs, bs, sk, srs, sbs, b, min(t0 + i, len - 1), g);
    f32x16 acc;
#pragma unroll
    for (int x = 0; x < 16; ++x) acc[x] = 0.f;
    const int nk = r_k / 16;
    for (int k = 0; k < nk; ++k)
        acc = kv_mfma<ADT>(__builtin_bit_cast(f16x8, qp[2 * k]), cp(k), acc);
    const int t = t0 + i;
    if (t < len) {
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const int h = h0 + acc_row(x, g);
            if (h < H) S[((int64_t)b * H + h) * tld + t] = scale * acc[x];
        }
    }
}

// ---- b, rotate_half: rebuild K = A_k[kvh] C_k^T per 32-token tile (features in the registers, tokens on the lanes), rotate, dot with q ----
// Feature d of the tile sits in register x of accumulator n with d = 32 n + acc_row(x, g), so the partner d + D/2 of the rotation is
// register x of accumulator n + D/64 of the SAME lane: the rotation needs no lane movement, the dot over d is a sum over registers plus
// one exchange between the two lane halves.  All heads of a KV group reuse the rotated tile.
template <int ADT, int D, bool Q8>
__global__ __launch_bounds__(256) void kv_scores_half_kernel(const uint16_t* __restrict__ q, const void* __restrict__ ck, int64_t rs, int64_t bs,
                                                             const float* __restrict__ sk, int64_t srs, int64_t sbs,
                                                             const int* __restrict__ lens, const uint16_t* __restrict__ Ak,
                                                             const float* __restrict__ cs, const float* __restrict__ sn, float* __restrict__ S,
                                                             float scale, int H, int group, int r_k, int Tmax, int tld) {
    constexpr int NT = D / 32, NP = D / 64;
    const int b = blockIdx.x, kvh = blockIdx.z, len = kv_len(lens, b, Tmax);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, i = lane & 31, g = lane >> 5;
    const int t0 = blockIdx.y * KV_TOK_TILE + wave * 32;
    if (t0 >= len) return;
    const int tc = min(t0 + i, len - 1);   // masked lanes work on a valid token and store nothing
    const KvTok<ADT, Q8> cp(ck, rs, bs, sk, srs, sbs, b, tc, g);
    const uint4* ap = (const uint4*)(Ak + ((int64_t)kvh * D + i) * r_k + 8 * g);
    const int64_t astep = (int64_t)32 * r_k / 8;   // 32 feature rows, in uint4
    f32x16 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int x = 0; x < 16; ++x) acc[n][x] = 0.f;
    const int nk = r_k / 16;
    for (int k = 0; k < nk; ++k) {
        const f16x8 c = cp(k);
#pragma unroll
        for (int n = 0; n < NT; ++n)
            acc[n] = kv_mfma<ADT>(__builtin_bit_cast(f16x8, ap[n * astep + 2 * k]), c, acc[n]);
    }
    // rotate in place: (lo, hi) <- (lo cos - hi sin, hi cos + lo sin), table row tc, column d of the low half
    const float* crow = cs + (int64_t)tc * (D / 2);
    const float* srow = sn + (int64_t)tc * (D / 2);
#pragma unroll
    for (int n = 0; n < NP; ++n)
#pragma unroll
        for (int x4 = 0; x4 < 4; ++x4) {
            const int d = 32 * n + 8 * x4 + 4 * g;
            const float4 c4 = *(const float4*)(crow + d), s4 = *(const float4*)(srow + d);
            const float cc[4] = {c4.x, c4.y, c4.z, c4.w}, ss[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float lo = acc[n][4 * x4 + u], hi = acc[n + NP][4 * x4 + u];
                acc[n][4 * x4 + u] = lo * cc[u] - hi * ss[u];
                acc[n + NP][4 * x4 + u] = hi * cc[u] + lo * ss[u];
            }
        }
    for (int hh = 0; hh < group; ++hh) {
        const int h = kvh * group + hh;
        const uint16_t* qh = q + ((int64_t)b * H + h) * D;
        float part = 0.f;
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int x4 = 0; x4 < 4; ++x4) {
                const uint2 qv = *(const uint2*)(qh + 32 * n + 8 * x4 + 4 * g);
                part += acc[n][4 * x4 + 0] * kv_to_f32<ADT>((uint16_t)(qv.x & 0xffffu));
                part += acc[n][4 * x4 + 1] * kv_to_f32<ADT>((uint16_t)(qv.x >> 16));
                part += acc[n][4 * x4 + 2] * kv_to_f32<ADT>((uint16_t)(qv.y & 0xffffu));
                part += acc[n][4 * x4 + 3] * kv_to_f32<ADT>((uint16_t)(qv.y >> 16));
            }
        const float other = __shfl_xor(part, 32, 64);
        const float tot = g == 0 ? part + other : other + part;   // lower half first in both halves
        if (g == 0 && t0 + i < len) S[((int64_t)b * H + h) * tld + t0 + i] = scale * tot;
    }
}

// scores_out [B, H, Tmax] <- S, zeros at t >= len[b]
__global__ __launch_bounds__(256) void kv_scores_copy_kernel(const float* __restrict__ S, const int* __restrict__ lens, float* __restrict__ out, int H,
                                                             int Tmax, int tld) {
    const int b = blockIdx.x / H, t = blockIdx.y * 256 + threadIdx.x;
    if (t >= Tmax) return;
    out[(int64_t)blockIdx.x * Tmax + t] = t < kv_len(lens, b, Tmax) ? S[(int64_t)blockIdx.x * tld + t] : 0.f;
}

// ---- c: one split of the tokens.  m, l and O~[32 heads, 32 ranks per wave] = p C_v ------------------------------------------------------
template <int ADT, bool Q8>
__global__ __launch_bounds__(256) void kv_pv_kernel(const float* __restrict__ S, const void* __restrict__ cv, int64_t rs, int64_t bs,
                                                    const float* __restrict__ sv, int64_t srs, int64_t sbs, const int* __restrict__ lens, float* __restrict__ ml, float* __restrict__ Op, int H, int r_v,
                                                    int Tmax, int hpad, int tld, int L, int ns) {
    const int nhb = hpad / 32;
    const int b = blockIdx.x / nhb, h0 = (blockIdx.x % nhb) * 32, s = blockIdx.y, len = kv_len(lens, b, Tmax);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, i = lane & 31, g = lane >> 5;
    const int start = s * L;
    if (start >= len) return;   // a split with no token: stage d skips it by the same test and reads nothing of it
    const int end = min(len, start + L);
    const int j0 = blockIdx.z * 128 + wave * 32;
    if (j0 >= r_v) return;
    const float* srow = S + ((int64_t)b * H + min(h0 + i, H - 1)) * tld;
    // pass 1: the split's maximum of head i (both lane halves scan half of the tokens)
    float m = -INFINITY;
    for (int tb = start; tb < end; tb += 16) {
        const int tt = tb + 8 * g;
        const float4 v0 = *(const float4*)(srow + tt), v1 = *(const float4*)(srow + tt + 4);
        const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (tt + u < end) m = fmaxf(m, v[u]);
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    // pass 2: p = ADT(exp(S - m)) is the A operand (row = head i, k = token), C_v the B operand (k = token, column = rank j0 + i)
    const KvCol<ADT, Q8> vcol(cv, rs, bs, sv, srs, sbs, b, min(j0 + i, r_v - 1));
    f32x16 acc;
#pragma unroll
    for (int x = 0; x < 16; ++x) acc[x] = 0.f;
    float l = 0.f;
    for (int tb = start; tb < end; tb += 16) {
        const int tt = tb + 8 * g;
        const float4 v0 = *(const float4*)(srow + tt), v1 = *(const float4*)(srow + tt + 4);
        const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        f16x8 pf, vf;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool live = tt + u < end;
            const uint16_t p = live ? kv_from_f32<ADT>(expf(v[u] - m)) : (uint16_t)0;   // l sums the ROUNDED p
            l += kv_to_f32<ADT>(p);
            pf[u] = __builtin_bit_cast(_Float16, p);
            const uint16_t c = vcol(min(tt + u, end - 1));
            vf[u] = __builtin_bit_cast(_Float16, (uint16_t)(live ? c : (uint16_t)0));
        }
        acc = kv_mfma<ADT>(pf, vf, acc);
    }
    const float lo = __shfl_xor(l, 32, 64);
    l = g == 0 ? l + lo : lo + l;
    const int64_t slot = ((int64_t)b * ns + s) * hpad;
    if (j0 + i < r_v) {
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            const int h = h0 + acc_row(x, g);
            if (h < H) Op[(slot + h) * r_v + j0 + i] = acc[x];
        }
    }
    if (blockIdx.z == 0 && wave == 0 && g == 0 && h0 + i < H) {
        ml[(slot + h0 + i) * 2] = m;
        ml[(slot + h0 + i) * 2 + 1] = l;
    }
}

// ---- d: merge the live splits in index order, up-project through A_v, add b_v, round once ----------------------------------------------
template <int ADT>
__global__ __launch_bounds__(256) void kv_combine_kernel(const float* __restrict__ ml, const float* __restrict__ Op, const int* __restrict__ lens,
                                                         const uint16_t* __restrict__ Av, const uint16_t* __restrict__ bv, uint16_t* __restrict__ out,
                                                         int H, int group, int D, int r_v, int Tmax, int hpad, int L, int ns) {
    extern __shared__ __attribute__((aligned(16))) float osum[];   // [r_v]
    const int b = blockIdx.x / H, h = blockIdx.x % H, kvh = h / group, tid = threadIdx.x, len = kv_len(lens, b, Tmax);
    uint16_t* orow = out + (int64_t)blockIdx.x * D;
    if (len <= 0) {   // nothing to attend to: a zero row, never 0 / 0
        if (tid < D) orow[tid] = 0;
        return;
    }
    const int live = (len + L - 1) / L;   // splits [0, live) hold tokens
    const int64_t slot0 = (int64_t)b * ns * hpad + h;
    float M = -INFINITY;
    for (int s = 0; s < live; ++s) M = fmaxf(M, ml[(slot0 + (int64_t)s * hpad) * 2]);
    float w[KV_MAX_SPLITS];
    float lsum = 0.f;
#pragma unroll
    for (int s = 0; s < KV_MAX_SPLITS; ++s) {
        w[s] = 0.f;
        if (s < live) {
            w[s] = expf(ml[(slot0 + (int64_t)s * hpad) * 2] - M);
            lsum += w[s] * ml[(slot0 + (int64_t)s * hpad) * 2 + 1];
        }
    }
    for (int j = tid; j < r_v; j += 256) {
        float o = 0.f;
#pragma unroll
        for (int s = 0; s < KV_MAX_SPLITS; ++s)
            if (s < live) o += w[s] * Op[(slot0 + (int64_t)s * hpad) * r_v + j];
        osum[j] = o;
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    const float inv = 1.f / lsum;
    for (int d = wave; d < D; d += 4) {
        const uint4* arow = (const uint4*)(Av + ((int64_t)kvh * D + d) * r_v);
        float acc = 0.f;
        for (int c = lane; c < r_v / 8; c += 64) {
            const uint4 a = arow[c];
            const float4 o0 = *(const float4*)(osum + 8 * c), o1 = *(const float4*)(osum + 8 * c + 4);
            acc += kv_to_f32<ADT>((uint16_t)(a.x & 0xffffu)) * o0.x;
            acc += kv_to_f32<ADT>((uint16_t)(a.x >> 16)) * o0.y;
            acc += kv_to_f32<ADT>((uint16_t)(a.y & 0xffffu)) * o0.z;
            acc += kv_to_f32<ADT>((uint16_t)(a.y >> 16)) * o0.w;
            acc += kv_to_f32<ADT>((uint16_t)(a.z & 0xffffu)) * o1.x;
            acc += kv_to_f32<ADT>((uint16_t)(a.z >> 16)) * o1.y;
            acc += kv_to_f32<ADT>((uint16_t)(a.w & 0xffffu)) * o1.z;
            acc += kv_to_f32<ADT>((uint16_t)(a.w >> 16)) * o1.w;
        }
        acc = wave_reduce_sum(acc);
        if (lane == 0) {
            float v = acc * inv;
            if (bv) v += kv_to_f32<ADT>(bv[kvh * D + d]);
            orow[d] = kv_from_f32<ADT>(v);
        }
    }
}

inline bool mis16(const void* p) { return ((uintptr_t)p & 15) != 0; }

// the argument rules shared by both entries; nothing here touches the device
int kv_check_common(const void* q, const void* ck, const void* lens, const void* Ak, const void* bk, const void* cs, const void* sn, int dtype,
                    int rope_mode, int64_t B, int64_t H, int64_t H_kv, int64_t D, int64_t r_k, int64_t Tmax, int64_t ck_rs, int64_t ck_bs,
                    const void* work, int64_t unit = 8) {   // unit: cache elements in 16 bytes (8 fp16 / bf16 values, 16 int8 codes)
    if (!q || !ck || !lens || !Ak || !work) return ASVD_E_BADARG;
    if (dtype != ASVD_F16 && dtype != ASVD_BF16) return ASVD_E_BADARG;
    if (rope_mode != ASVD_KV_ROPE_NONE && rope_mode != ASVD_KV_ROPE_HALF) return ASVD_E_BADARG;
    if (D != 64 && D != 128) return ASVD_E_BADARG;
    if (B < 1 || B > (1 << 20) || H < 1 || H > 4096 || H_kv < 1 || H % H_kv || Tmax < 1 || Tmax > (1 << 22)) return ASVD_E_BADARG;
    if (r_k < 16 || r_k % 16 || r_k > KV_MAX_RANK) return ASVD_E_BADARG;
    if (ck_rs < r_k || ck_rs % unit || ck_bs % unit || ck_bs < 0 || (B > 1 && ck_bs < Tmax * ck_rs)) return ASVD_E_BADARG;
    if (mis16(q) || mis16(ck) || mis16(Ak) || mis16(work) || ((uintptr_t)lens & 3)) return ASVD_E_BADARG;
    if (rope_mode == ASVD_KV_ROPE_HALF) {
        if (!cs || !sn || mis16(cs) || mis16(sn) || bk) return ASVD_E_BADARG;   // a key bias does not commute with the rotation's absorbed form
    }
    return ASVD_OK;
}

// the second cache of the whole op
int kv_check_values(const void* cv, const void* Av, const void* out, int64_t B, int64_t r_v, int64_t Tmax, int64_t cv_rs, int64_t cv_bs, int64_t unit) {
    if (!cv || !Av || !out || mis16(cv) || mis16(Av) || mis16(out)) return ASVD_E_BADARG;
    if (r_v < 16 || r_v % 16 || r_v > KV_MAX_RANK) return ASVD_E_BADARG;
    if (cv_rs < r_v || cv_rs % unit || cv_bs % unit || cv_bs < 0 || (B > 1 && cv_bs < Tmax * cv_rs)) return ASVD_E_BADARG;
    return ASVD_OK;
}

// the scales of an int8 cache: fp32 [B, Tmax, >= ceil(r / 32)], strides in floats
int kv_check_scales(const void* s, int64_t B, int64_t r, int64_t Tmax, int64_t s_rs, int64_t s_bs) {
    if (!s || ((uintptr_t)s & 3)) return ASVD_E_BADARG;
    if (s_rs < kv_q8_groups(r) || s_bs < 0 || (B > 1 && s_bs < Tmax * s_rs)) return ASVD_E_BADARG;
    return ASVD_OK;
}

template <int ADT, bool Q8>
int kv_scores_launch(const KvPlan& p, const void* q, const void* ck, const void* lens, const void* Ak, const void* cs, const void* sn, int rope_mode,
                     float scale, int64_t B, int64_t H, int64_t H_kv, int64_t D, int64_t r_k, int64_t Tmax, int64_t ck_rs, int64_t ck_bs, const float* sk,
                     int64_t sk_rs, int64_t sk_bs, void* work, hipStream_t st) {
    uint16_t* qt = (uint16_t*)((char*)work + p.off_qt);
    float* S = (float*)((char*)work + p.off_s);
    const int group = (int)(H / H_kv), ntile = (int)ceil_div64(Tmax, KV_TOK_TILE);
    if (rope_mode == ASVD_KV_ROPE_NONE) {
        hipLaunchKernelGGL((kv_qtilde_kernel<ADT>), dim3((unsigned)(B * H), (unsigned)ceil_div64(r_k, 256)), dim3(256), 0, st, (const uint16_t*)q,
                           (const uint16_t*)Ak, qt, (int)H, group, (int)D, (int)r_k, (int)p.hpad);
        hipLaunchKernelGGL((kv_scores_none_kernel<ADT, Q8>), dim3((unsigned)B, ntile, (unsigned)(p.hpad / 32)), dim3(256), 0, st, (const uint16_t*)qt,
                           ck, ck_rs, ck_bs, sk, sk_rs, sk_bs, (const int*)lens, S, scale, (int)H, (int)r_k, (int)Tmax, (int)p.hpad, (int)p.tld);
    } else if (D == 64) {
        hipLaunchKernelGGL((kv_scores_half_kernel<ADT, 64, Q8>), dim3((unsigned)B, ntile, (unsigned)H_kv), dim3(256), 0, st, (const uint16_t*)q,
                           ck, ck_rs, ck_bs, sk, sk_rs, sk_bs, (const int*)lens, (const uint16_t*)Ak, (const float*)cs, (const float*)sn, S, scale,
                           (int)H, group, (int)r_k, (int)Tmax, (int)p.tld);
    } else {
        hipLaunchKernelGGL((kv_scores_half_kernel<ADT, 128, Q8>), dim3((unsigned)B, ntile, (unsigned)H_kv), dim3(256), 0, st, (const uint16_t*)q,
                           ck, ck_rs, ck_bs, sk, sk_rs, sk_bs, (const int*)lens, (const uint16_t*)Ak, (const float*)cs, (const float*)sn, S, scale,
                           (int)H, group, (int)r_k, (int)Tmax, (int)p.tld);
    }
    ASVD_HIP_CHECK(hipGetLastError());
    return ASVD_OK;
}

template <bool Q8>
int kv_scores_entry(const void* q, const void* ck, const void* sk, const void* lens, const void* Ak, const void* bk, const void* cos_tab,
                    const void* sin_tab, int dtype, int rope_mode, float scale, int64_t B, int64_t H, int64_t H_kv, int64_t D, int64_t r_k, int64_t Tmax,
                    int64_t ck_row_stride, int64_t ck_batch_stride, int64_t sk_row_stride, int64_t sk_batch_stride, void* scores_out, void* work,
                    size_t work_bytes, void* stream) {
    int rc = kv_check_common(q, ck, lens, Ak, bk, cos_tab, sin_tab, dtype, rope_mode, B, H, H_kv, D, r_k, Tmax, ck_row_stride, ck_batch_stride, work,
                             Q8 ? 16 : 8);
    if (rc == ASVD_OK && Q8) rc = kv_check_scales(sk, B, r_k, Tmax, sk_row_stride, sk_batch_stride);
    if (rc != ASVD_OK) return rc;
    if (scores_out && ((uintptr_t)scores_out & 3)) return ASVD_E_BADARG;
    const KvPlan p = kv_plan(B, H, Tmax, r_k, 16);
    if (work_bytes < p.off_ml) return ASVD_E_WORKSPACE;   // q~ and S only
    const int lrc = dtype == ASVD_BF16
                        ? kv_scores_launch<ASVD_BF16, Q8>(p, q, ck, lens, Ak, cos_tab, sin_tab, rope_mode, scale, B, H, H_kv, D, r_k, Tmax, ck_row_stride,
                                                          ck_batch_stride, (const float*)sk, sk_row_stride, sk_batch_stride, work, (hipStream_t)stream)
                        : kv_scores_launch<ASVD_F16, Q8>(p, q, ck, lens, Ak, cos_tab, sin_tab, rope_mode, scale, B, H, H_kv, D, r_k, Tmax, ck_row_stride,
                                                         ck_batch_stride, (const float*)sk, sk_row_stride, sk_batch_stride, work, (hipStream_t)stream);
    if (lrc != ASVD_OK) return lrc;
    if (scores_out) {
        hipLaunchKernelGGL(kv_scores_copy_kernel, dim3((unsigned)(B * H), (unsigned)ceil_div64(Tmax, 256)), dim3(256), 0, (hipStream_t)stream,
                           (const float*)((char*)work + p.off_s), (const int*)lens, (float*)scores_out, (int)H, (int)Tmax, (int)p.tld);
        ASVD_HIP_CHECK(hipGetLastError());
    }
    return ASVD_OK;
}

// stages a - d of the whole op on checked arguments
template <int ADT, bool Q8>
int kv_decode_go(const KvPlan& p, const void* q, const void* ck, const void* cv, const void* sk, const void* sv, const void* lens, const void* Ak,
                 const void* Av, const void* bv, const void* cos_tab, const void* sin_tab, int rope_mode, float scale, int64_t B, int64_t H, int64_t H_kv,
                 int64_t D, int64_t r_k, int64_t r_v, int64_t Tmax, int64_t ck_row_stride, int64_t ck_batch_stride, int64_t cv_row_stride,
                 int64_t cv_batch_stride, int64_t sk_row_stride, int64_t sk_batch_stride, int64_t sv_row_stride, int64_t sv_batch_stride, void* out,
                 void* work, hipStream_t st) {
    const int lrc = kv_scores_launch<ADT, Q8>(p, q, ck, lens, Ak, cos_tab, sin_tab, rope_mode, scale, B, H, H_kv, D, r_k, Tmax, ck_row_stride,
                                              ck_batch_stride, (const float*)sk, sk_row_stride, sk_batch_stride, work, st);
    if (lrc != ASVD_OK) return lrc;
    const float* S = (const float*)((char*)work + p.off_s);
    float* ml = (float*)((char*)work + p.off_ml);
    float* Op = (float*)((char*)work + p.off_o);
    hipLaunchKernelGGL((kv_pv_kernel<ADT, Q8>), dim3((unsigned)(B * (p.hpad / 32)), (unsigned)p.n_splits, (unsigned)ceil_div64(r_v, 128)), dim3(256), 0, st,
                       S, cv, cv_row_stride, cv_batch_stride, (const float*)sv, sv_row_stride, sv_batch_stride, (const int*)lens, ml, Op, (int)H, (int)r_v,
                       (int)Tmax, (int)p.hpad, (int)p.tld, (int)p.split_len, (int)p.n_splits);
    hipLaunchKernelGGL((kv_combine_kernel<ADT>), dim3((unsigned)(B * H)), dim3(256), (size_t)r_v * sizeof(float), st, (const float*)ml, (const float*)Op,
                       (const int*)lens, (const uint16_t*)Av, (const uint16_t*)bv, (uint16_t*)out, (int)H, (int)(H / H_kv), (int)D, (int)r_v,
                       (int)Tmax, (int)p.hpad, (int)p.split_len, (int)p.n_splits);
    ASVD_HIP_CHECK(hipGetLastError());
    return ASVD_OK;
}

template <bool Q8>
int kv_decode_entry(const void* q, const void* ck, const void* cv, const void* sk, const void* sv, const void* lens, const void* Ak, const void* Av,
                    const void* bk, const void* bv, const void* cos_tab, const void* sin_tab, int dtype, int rope_mode, float scale, int64_t B, int64_t H,
                    int64_t H_kv, int64_t D, int64_t r_k, int64_t r_v, int64_t Tmax, int64_t ck_row_stride, int64_t ck_batch_stride,
                    int64_t cv_row_stride, int64_t cv_batch_stride, int64_t sk_row_stride, int64_t sk_batch_stride, int64_t sv_row_stride,
                    int64_t sv_batch_stride, void* out, void* work, size_t work_bytes, void* stream) {
    const int64_t unit = Q8 ? 16 : 8;
    int rc = kv_check_common(q, ck, lens, Ak, bk, cos_tab, sin_tab, dtype, rope_mode, B, H, H_kv, D, r_k, Tmax, ck_row_stride, ck_batch_stride, work, unit);
    if (rc == ASVD_OK) rc = kv_check_values(cv, Av, out, B, r_v, Tmax, cv_row_stride, cv_batch_stride, unit);
    if (rc == ASVD_OK && Q8) rc = kv_check_scales(sk, B, r_k, Tmax, sk_row_stride, sk_batch_stride);
    if (rc == ASVD_OK && Q8) rc = kv_check_scales(sv, B, r_v, Tmax, sv_row_stride, sv_batch_stride);
    if (rc != ASVD_OK) return rc;
    const KvPlan p = kv_plan(B, H, Tmax, r_k, r_v);
    if (work_bytes < p.total) return ASVD_E_WORKSPACE;
    if (dtype == ASVD_BF16)
        return kv_decode_go<ASVD_BF16, Q8>(p, q, ck, cv, sk, sv, lens, Ak, Av, bv, cos_tab, sin_tab, rope_mode, scale, B, H, H_kv, D, r_k, r_v, Tmax,
                                           ck_row_stride, ck_batch_stride, cv_row_stride, cv_batch_stride, sk_row_stride, sk_batch_stride, sv_row_stride,
                                           sv_batch_stride, out, work, (hipStream_t)stream);
    return kv_decode_go<ASVD_F16, Q8>(p, q, ck, cv, sk, sv, lens, Ak, Av, bv, cos_tab, sin_tab, rope_mode, scale, B, H, H_kv, D, r_k, r_v, Tmax,
                                      ck_row_stride, ck_batch_stride, cv_row_stride, cv_batch_stride, sk_row_stride, sk_batch_stride, sv_row_stride,
                                      sv_batch_stride, out, work, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int asvd_lowrank_kv_plan(int64_t B, int64_t H, int64_t Tmax, int64_t* token_tile, int64_t* split_len, int64_t* n_splits) {
    if (B < 1 || H < 1 || Tmax < 1 || !token_tile || !split_len || !n_splits) return ASVD_E_BADARG;
    const KvPlan p = kv_plan(B, H, Tmax, 16, 16);
    *token_tile = 32;
    *split_len = p.split_len;
    *n_splits = p.n_splits;
    return ASVD_OK;
}

int asvd_lowrank_kv_worksize(int64_t B, int64_t H, int64_t Tmax, int64_t r_k, int64_t r_v, size_t* bytes) {
    if (B < 1 || H < 1 || Tmax < 1 || r_k < 16 || r_k % 16 || r_v < 16 || r_v % 16 || !bytes) return ASVD_E_BADARG;
    *bytes = kv_plan(B, H, Tmax, r_k, r_v).total;
    return ASVD_OK;
}

// K22: the _a16 entries take dtype ASVD_F16 or ASVD_BF16 (the type of q, A_k, A_v, the biases, the output and of an unquantised cache);
// the entries without the suffix keep their fp16-only rule and forward
int asvd_lowrank_kv_scores_a16(const void* q, const void* ck, const void* lens, const void* Ak, const void* bk, const void* cos_tab,
                               const void* sin_tab, int dtype, int rope_mode, float scale, int64_t B, int64_t H, int64_t H_kv, int64_t D, int64_t r_k,
                               int64_t Tmax, int64_t ck_row_stride, int64_t ck_batch_stride, void* scores_out, void* work, size_t work_bytes,
                               void* stream) {
    return kv_scores_entry<false>(q, ck, nullptr, lens, Ak, bk, cos_tab, sin_tab, dtype, rope_mode, scale, B, H, H_kv, D, r_k, Tmax, ck_row_stride,
                                  ck_batch_stride, 0, 0, scores_out, work, work_bytes, stream);
}

int asvd_lowrank_kv_decode_a16(const void* q, const void* ck, const void* cv, const void* lens, const void* Ak, const void* Av, const void* bk,
                               const void* bv, const void* cos_tab, const void* sin_tab, int dtype, int rope_mode, float scale, int64_t B, int64_t H,
                               int64_t H_kv, int64_t D, int64_t r_k, int64_t r_v, int64_t Tmax, int64_t ck_row_stride, int64_t ck_batch_stride,
                               int64_t cv_row_stride, int64_t cv_batch_stride, void* out, void* work, size_t work_bytes, void* stream) {
    return kv_decode_entry<false>(q, ck, cv, nullptr, nullptr, lens, Ak, Av, bk, bv, cos_tab, sin_tab, dtype, rope_mode, scale, B, H, H_kv, D, r_k, r_v,
                                  Tmax, ck_row_stride, ck_batch_stride, cv_row_stride, cv_batch_stride, 0, 0, 0, 0, out, work, work_bytes, stream);
}

// K21: the same stages on an int8 cache; ck / cv are codes (strides in bytes), sk / sv their fp32 group scales (strides in floats)
int asvd_lowrank_kv_scores_q8_a16(const void* q, const void* ck, const void* sk, const void* lens, const void* Ak, const void* bk, const void* cos_tab,
                                  const void* sin_tab, int dtype, int rope_mode, float scale, int64_t B, int64_t H, int64_t H_kv, int64_t D,
                                  int64_t r_k, int64_t Tmax, int64_t ck_row_stride, int64_t ck_batch_stride, int64_t sk_row_stride,
                                  int64_t sk_batch_stride, void* scores_out, void* work, size_t work_bytes, void* stream) {
    return kv_scores_entry<true>(q, ck, sk, lens, Ak, bk, cos_tab, sin_tab, dtype, rope_mode, scale, B, H, H_kv, D, r_k, Tmax, ck_row_stride,
                                 ck_batch_stride, sk_row_stride, sk_batch_stride, scores_out, work, work_bytes, stream);
}

int asvd_lowrank_kv_decode_q8_a16(const void* q, const void* ck, const void* cv, const void* sk, const void* sv, const void* lens, const void* Ak,
                                  const void* Av, const void* bk, const void* bv, const void* cos_tab, const void* sin_tab, int dtype, int rope_mode,
                                  float scale, int64_t B, int64_t H, int64_t H_kv, int64_t D, int64_t r_k, int64_t r_v, int64_t Tmax,
                                  int64_t ck_row_stride, int64_t ck_batch_stride, int64_t cv_row_stride, int64_t cv_batch_stride,
                                  int64_t sk_row_stride, int64_t sk_batch_stride, int64_t sv_row_stride, int64_t sv_batch_stride, void* out, void* work,
                                  size_t work_bytes, void* stream) {
    return kv_decode_entry<true>(q, ck, cv, sk, sv, lens, Ak, Av, bk, bv, cos_tab, sin_tab, dtype, rope_mode, scale, B, H, H_kv, D, r_k, r_v, Tmax,
                                 ck_row_stride, ck_batch_stride, cv_row_stride, cv_batch_stride, sk_row_stride, sk_batch_stride, sv_row_stride,
                                 sv_batch_stride, out, work, work_bytes, stream);
}

int asvd_lowrank_kv_scores(const void* q, const void* ck, const void* lens, const void* Ak, const void* bk, const void* cos_tab, const void* sin_tab,
                           int dtype, int rope_mode, float scale, int64_t B, int64_t H, int64_t H_kv, int64_t D, int64_t r_k, int64_t Tmax,
                           int64_t ck_row_stride, int64_t ck_batch_stride, void* scores_out, void* work, size_t work_bytes, void* stream) {
    if (dtype != ASVD_F16) return ASVD_E_BADARG;
    return asvd_lowrank_kv_scores_a16(q, ck, lens, Ak, bk, cos_tab, sin_tab, dtype, rope_mode, scale, B, H, H_kv, D, r_k, Tmax, ck_row_stride,
                                      ck_batch_stride, scores_out, work, work_bytes, stream);
}

int asvd_lowrank_kv_decode(const void* q, const void* ck, const void* cv, const void* lens, const void* Ak, const void* Av, const void* bk,
                           const void* bv, const void* cos_tab, const void* sin_tab, int dtype, int rope_mode, float scale, int64_t B, int64_t H,
                           int64_t H_kv, int64_t D, int64_t r_k, int64_t r_v, int64_t Tmax, int64_t ck_row_stride, int64_t ck_batch_stride,
                           int64_t cv_row_stride, int64_t cv_batch_stride, void* out, void* work, size_t work_bytes, void* stream) {
    if (dtype != ASVD_F16) return ASVD_E_BADARG;
    return asvd_lowrank_kv_decode_a16(q, ck, cv, lens, Ak, Av, bk, bv, cos_tab, sin_tab, dtype, rope_mode, scale, B, H, H_kv, D, r_k, r_v, Tmax,
                                      ck_row_stride, ck_batch_stride, cv_row_stride, cv_batch_stride, out, work, work_bytes, stream);
}

int asvd_lowrank_kv_scores_q8(const void* q, const void* ck, const void* sk, const void* lens, const void* Ak, const void* bk, const void* cos_tab,
                              const void* sin_tab, int dtype, int rope_mode, float scale, int64_t B, int64_t H, int64_t H_kv, int64_t D, int64_t r_k,
                              int64_t Tmax, int64_t ck_row_stride, int64_t ck_batch_stride, int64_t sk_row_stride, int64_t sk_batch_stride,
                              void* scores_out, void* work, size_t work_bytes, void* stream) {
    if (dtype != ASVD_F16) return ASVD_E_BADARG;
    return asvd_lowrank_kv_scores_q8_a16(q, ck, sk, lens, Ak, bk, cos_tab, sin_tab, dtype, rope_mode, scale, B, H, H_kv, D, r_k, Tmax, ck_row_stride,
                                         ck_batch_stride, sk_row_stride, sk_batch_stride, scores_out, work, work_bytes, stream);
}

int asvd_lowrank_kv_decode_q8(const void* q, const void* ck, const void* cv, const void* sk, const void* sv, const void* lens, const void* Ak,
                              const void* Av, const void* bk, const void* bv, const void* cos_tab, const void* sin_tab, int dtype, int rope_mode,
                              float scale, int64_t B, int64_t H, int64_t H_kv, int64_t D, int64_t r_k, int64_t r_v, int64_t Tmax,
                              int64_t ck_row_stride, int64_t ck_batch_stride, int64_t cv_row_stride, int64_t cv_batch_stride, int64_t sk_row_stride,
                              int64_t sk_batch_stride, int64_t sv_row_stride, int64_t sv_batch_stride, void* out, void* work, size_t work_bytes,
                              void* stream) {
    if (dtype != ASVD_F16) return ASVD_E_BADARG;
    return asvd_lowrank_kv_decode_q8_a16(q, ck, cv, sk, sv, lens, Ak, Av, bk, bv, cos_tab, sin_tab, dtype, rope_mode, scale, B, H, H_kv, D, r_k, r_v,
                                         Tmax, ck_row_stride, ck_batch_stride, cv_row_stride, cv_batch_stride, sk_row_stride, sk_batch_stride,
                                         sv_row_stride, sv_batch_stride, out, work, work_bytes, stream);
}

}  // extern "C"
