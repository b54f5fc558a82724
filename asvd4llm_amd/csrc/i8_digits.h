// i8_digits.h — what the int8 digit-product kernels share (included by svd_jacobi.hip inside its anonymous namespace, ahead of gram_i8.h, nn_gemm_i8.h
// and snapshot_i8.h): the exponent rules, the balanced radix-256 digit packer, the block decode of an upper triangle and the tile main loop.
#pragma once

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int GI_BAD = 0x7fffffff;   // exponent sentinel: the column holds Inf / NaN
constexpr int GI_ZERO = -0x40000000; // exponent of an all-zero column (digits are all zero, the scale does not matter)

// E with max 2^-E < 127/128, from the bit pattern of the largest magnitude (magnitudes of finite floats order like their bit patterns; Inf / NaN
// patterns are above all of them)
__device__ __forceinline__ int gi_exp_of_bits(unsigned mx) {
    if (mx >= 0x7f800000u) return GI_BAD;
    if (mx == 0u) return GI_ZERO;
    int e2;
    const float f = frexpf(__uint_as_float(mx), &e2);  // mx = f 2^e2, f in [0.5, 1)
    return e2 + (f >= 127.0f / 128.0f ? 1 : 0);
}

// Maxima of |x| 2^shift over a row / column are taken on KEYS (exponent + shift in the high bits, mantissa below: ordered like the scaled magnitudes,
// with no intermediate overflow or underflow); 0 = all zero, 0xffffffff = Inf / NaN met.
__device__ __forceinline__ unsigned gi_key(float x, int shift) {
    const unsigned a = __float_as_uint(x) & 0x7fffffffu;
    if (a >= 0x7f800000u) return 0xffffffffu;
    if (a == 0u) return 0u;
    int e;
    const float f = frexpf(__uint_as_float(a), &e);                 // f in [0.5, 1)
    const unsigned mant = (unsigned)ldexpf(f, 24) - 0x800000u;      // 23 bits, exact
    const int ee = min(max(e + shift + 256, 1), 510);                // nine bits; beyond 2^+-254 of the scale the order no longer matters
    return ((unsigned)ee << 23) | mant;
}
__device__ __forceinline__ int gi_exp_of_key(unsigned key) {       // E with (max) 2^-E < 127/128
    if (key == 0xffffffffu) return GI_BAD;
    if (key == 0u) return GI_ZERO;
    return (int)(key >> 23) - 256 + ((key & 0x7fffffu) >= 0x7e0000u ? 1 : 0);
}

// value of one unit of a 24-bit integer under exponent E
__device__ __forceinline__ double gi_scale(int E) { return E == GI_BAD ? __builtin_nan("") : (E == GI_ZERO ? 0.0 : ldexp(1.0, E - 23)); }

// Digit packer: the three balanced radix-256 digits of t = d0 2^16 + d1 2^8 + d2, |t| <= 127 * 2^16 (d0 in [-127, 127], d1, d2 in [-128, 127]), go
// into byte i (0..15) of the packed words w0 / w1 / w2 (zero before the first call); gi_store_digits writes the 16-byte piece at pb of each plane.
__device__ __forceinline__ void gi_pack_digits(int t, int i, unsigned (&w0)[4], unsigned (&w1)[4], unsigned (&w2)[4]) {
    const int d2 = (int)(signed char)(t & 0xff);
    const int t1 = (t - d2) >> 8;
    const int d1 = (int)(signed char)(t1 & 0xff);
    const int d0 = (t1 - d1) >> 8;
    w0[i >> 2] |= (unsigned)(d0 & 0xff) << (8 * (i & 3));
    w1[i >> 2] |= (unsigned)(d1 & 0xff) << (8 * (i & 3));
    w2[i >> 2] |= (unsigned)(d2 & 0xff) << (8 * (i & 3));
}
__device__ __forceinline__ void gi_store_digits(signed char* pb, int64_t plane_stride, const unsigned (&w0)[4], const unsigned (&w1)[4], const unsigned (&w2)[4]) {
    *(uint4*)(pb) = make_uint4(w0[0], w0[1], w0[2], w0[3]);
    *(uint4*)(pb + plane_stride) = make_uint4(w1[0], w1[1], w1[2], w1[3]);
    *(uint4*)(pb + 2 * plane_stride) = make_uint4(w2[0], w2[1], w2[2], w2[3]);
}

// Block (Ib <= Jb) of the upper triangle of nt x nt blocks for this workgroup of a (nt (nt + 1) / 2, ...) grid, in XCD-aware order: consecutive
// workgroup ids go round-robin over the 8 XCDs; give every XCD a contiguous run of blocks (they share I panels in its L2) (a block count that is
// not a multiple of 8 keeps the plain order: correct, merely less local).  Row runs per XCD; 4 x 8 groups of blocks per XCD and the plain order
// were measured against it (tools/bench_i8_gemm.py, round 6) and removed.
__device__ __forceinline__ void gi_tri_block(int nt, int& Ib, int& Jb) {
    const int total = gridDim.x;
    int rem = (total & 7) ? (int)blockIdx.x : (int)((blockIdx.x & 7) * (total >> 3) + (blockIdx.x >> 3));
    Ib = 0;
    while (rem >= nt - Ib) { rem -= nt - Ib; ++Ib; }
    Jb = Ib + rem;
}

// The tile main loop: acc[t][s] = sum over the digit pairs a + c = s < NW of (digit a of A panel 4 Ib + 2 (w >> 2) + t)^T (digit c of B panel
// 4 Jb + (w & 3)), exactly, for wave w of a workgroup of 512 threads = one 128 x 128 block (64 x 32 per wave: 2 tiles x NW weights x 16
// accumulator registers, two waves per SIMD).  A plane set is [digit a][panel P][16-index group kg][column c][16 bytes = reduction indices] with
// `stride` bytes per digit: one (P, kg) piece of a digit is 512 contiguous bytes, and two consecutive pieces are the A (or B) operand of one
// v_mfma_i32_32x32x32_i8 of a wave: lane l = 32 (kg & 1) + c reads its 16 bytes at offset 16 l.  Panels >= npA / npB read as zero.  A stage = 64
// reduction indices (kgs is a multiple of 4) of the four A panels and the four B panels, three digits each: 2 x 24 KB through LDS in the planes'
// own order (linear 16-byte pieces: no bank conflicts either way), double buffered in lds[2 x GI_STAGE_BYTES]; per stage and wave 2 x 18 (NW = 5:
// all nine digit products) or 2 x 16 (NW = 4: the product of the two lowest digits dropped) matrix instructions on 2 x 9 operand reads.
// D[i][j] of acc[t][s]: j = lane & 31 (B operand), i = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (A operand).
// Forced inline, and acc indexed with compile-time indices only: a call or a runtime index would put the accumulators in scratch.
constexpr int GI_STAGE_BYTES = 2 * 3 * 4 * 4 * 512;  // side, digit, panel, row group
template <int NW>
__device__ __forceinline__ void gi_tile_loop(const signed char* __restrict__ plA, int64_t strideA, int npA, const signed char* __restrict__ plB,
                                             int64_t strideB, int npB, int Ib, int Jb, int kgs, unsigned char* lds, i32x16 (&acc)[2][NW]) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wi = w >> 2, wj = w & 3;
    // loader: piece q of a stage (16 bytes), q = round * 512 + tid, in LDS order [side][digit][panel][row group][column]
    const unsigned char* gsrc[6];
    bool gok[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const int q = r * 512 + tid;
        const int side = q / 1536, qq = q % 1536;
        const int a = (qq >> 7) >> 2, p4 = (qq >> 7) & 3, within = qq & 127;  // within: row group (2 bits) x column (5 bits)
        const int P = 4 * (side ? Jb : Ib) + p4;
        gok[r] = P < (side ? npB : npA);
        gsrc[r] = (const unsigned char*)(side ? plB : plA) + (int64_t)a * (side ? strideB : strideA) + (int64_t)(gok[r] ? P : 0) * kgs * 512 + within * 16;
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < NW; ++s)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][s][i] = 0;

    const int nstage = kgs >> 2;
    uint4 stg[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) stg[r] = gok[r] ? *(const uint4*)(gsrc[r]) : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 6; ++r) *(uint4*)(lds + (r * 512 + tid) * 16) = stg[r];
    __syncthreads();
    for (int st = 0; st < nstage; ++st) {
        const unsigned char* cur = lds + (st & 1) * GI_STAGE_BYTES;
        if (st + 1 < nstage) {
#pragma unroll
            for (int r = 0; r < 6; ++r) stg[r] = gok[r] ? *(const uint4*)(gsrc[r] + (int64_t)(st + 1) * 2048) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            i32x4 fa[2][3], fb[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    fa[t][a] = *(const i32x4*)(cur + (((0 * 3 + a) * 4 + 2 * wi + t) * 4 + 2 * ks) * 512 + lane * 16);
                fb[a] = *(const i32x4*)(cur + (((1 * 3 + a) * 4 + wj) * 4 + 2 * ks) * 512 + lane * 16);
            }
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int t = 0; t < 2; ++t)
                        if (a + c < NW) acc[t][a + c] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[t][a], fb[c], acc[t][a + c], 0, 0, 0);
        }
        if (st + 1 < nstage) {
            unsigned char* nxt = lds + ((st + 1) & 1) * GI_STAGE_BYTES;
#pragma unroll
            for (int r = 0; r < 6; ++r) *(uint4*)(nxt + (r * 512 + tid) * 16) = stg[r];
        }
        __syncthreads();
    }
}
