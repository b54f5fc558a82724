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
// v_mfma_i32_32x32x32_i8 of a wave: lane l = 32 (kg & 1) + c reads its 16 bytes at offset 16 l.
// Panels >= npA / npB read as the LAST existing panel (npA, npB >= 1): the accumulators of such a panel hold products of real digits that belong
// nowhere, and every caller drops them — gram_i8_kernel and fullcheck_i8_kernel by `if (J >= nb) return` / `if (I > J || I >= nb) continue`,
// nn_gemm_i8_kernel by `if (j >= k) return` (k <= 32 jps); on its A side it tests rows only against the matrix, so launch_nn_i8 gives it segments
// of a multiple of four panels (checked there), which hold no clamped panel.  A caller
// that stores a block of a panel >= np must zero it itself.
// A stage = 64 reduction indices (kgs is a multiple of 4) of the four A panels and the four B panels, three digits each: 2 x 24 KB in LDS in the
// planes' own order (linear 16-byte pieces: no bank conflicts either way).  The stages go through a ring of GI_SLOTS = 3 slots filled by
// global_load_lds_dwordx4 (six per thread and stage, 1 KiB contiguous per wave instruction; no staging registers, no LDS stores): stage st + 2 is
// requested while stage st is in the matrix pipe.  Per stage: wait for the wave's OWN loads of stage st (vmcnt(6): the six of stage st + 1 stay in
// flight; vmcnt(0) on the last stage), one raw s_barrier (after it every wave's part of stage st is in LDS and every wave has finished reading
// stage st - 1), request stage st + 2 into the slot of stage st - 1, then 2 x 9 operand reads and 2 x 18 (NW = 5: all nine digit products) or 2 x 16
// (NW = 4: the product of the two lowest digits dropped) matrix instructions.  No __syncthreads() in the loop (it would drain the loads in flight),
// no register-destination global load until the loop's last vmcnt(0), and all LDS in the caller's one dynamic array of GI_LDS_BYTES.
// D[i][j] of acc[t][s]: j = lane & 31 (B operand), i = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (A operand).
// Forced inline, and acc indexed with compile-time indices only: a call or a runtime index would put the accumulators in scratch.
constexpr int GI_STAGE_BYTES = 2 * 3 * 4 * 4 * 512;  // side, digit, panel, row group
constexpr int GI_SLOTS = 3;
constexpr int GI_LDS_BYTES = GI_SLOTS * GI_STAGE_BYTES;  // dynamic LDS of every kernel that runs gi_tile_loop

// piece q = r * 512 + tid of a stage in LDS order [side][digit][panel][row group][column]: r = 3 side + digit, tid = 128 panel + 32 row group + column
__device__ __forceinline__ void gi_request_stage(const unsigned char* gA, int64_t strideA, const unsigned char* gB, int64_t strideB, unsigned char* wave_dst) {
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const unsigned char* src = r < 3 ? gA + r * strideA : gB + (r - 3) * strideB;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)(wave_dst + r * 8192), 16, 0, 0);
    }
}

// One stage out of the slot at `cur`; REQ: stage st + 2 is requested into `wave_fill` behind the first matrix instructions.  Order in the wave's
// instruction stream, pinned with sched_group_barrier: the nine operand reads of the first half-stage, then its matrix instructions with the six
// loads and the nine reads of the second half-stage one by one between them, then the rest.  What the compiler makes of it: lgkmcnt(0) after the
// first nine reads, so the first matrix instruction of a stage still waits for that burst behind the barrier, and a second lgkmcnt(0) half-way,
// by which the second half-stage's reads have long returned; only those are hidden.
template <int NW, bool REQ>
__device__ __forceinline__ void gi_stage(const unsigned char* cur, int lane, int wi, int wj, const unsigned char* gA, int64_t strideA, const unsigned char* gB,
                                         int64_t strideB, unsigned char* wave_fill, i32x16 (&acc)[2][NW]) {
    i32x4 fa[2][2][3], fb[2][3];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        if (ks == 1 && REQ) gi_request_stage(gA, strideA, gB, strideB, wave_fill);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int t = 0; t < 2; ++t) fa[ks][t][a] = *(const i32x4*)(cur + (((0 * 3 + a) * 4 + 2 * wi + t) * 4 + 2 * ks) * 512 + lane * 16);
            fb[ks][a] = *(const i32x4*)(cur + (((1 * 3 + a) * 4 + wj) * 4 + 2 * ks) * 512 + lane * 16);
        }
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    if (a + c < NW) acc[t][a + c] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[ks][t][a], fb[ks][c], acc[t][a + c], 0, 0, 0);
    constexpr int NM = NW >= 5 ? 18 : 16;  // matrix instructions per half-stage
    __builtin_amdgcn_sched_group_barrier(0x100, 9, 0);  // DS read
    if (REQ) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
            __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);  // VMEM
        }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
    __builtin_amdgcn_sched_group_barrier(0x008, 2 * NM - 9 - (REQ ? 6 : 0), 0);
}

template <int NW>
__device__ __forceinline__ void gi_tile_loop(const signed char* __restrict__ plA, int64_t strideA, int npA, const signed char* __restrict__ plB,
                                             int64_t strideB, int npB, int Ib, int Jb, int kgs, unsigned char* lds, i32x16 (&acc)[2][NW]) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wi = w >> 2, wj = w & 3;
    // loader: this thread's 16 bytes of panel tid >> 7 of either side, stage 0; a stage further on is 2048 bytes further on
    const int p4 = tid >> 7, within = tid & 127;  // within: row group (2 bits) x column (5 bits)
    const unsigned char* gA = (const unsigned char*)plA + (int64_t)min(4 * Ib + p4, npA - 1) * kgs * 512 + within * 16;
    const unsigned char* gB = (const unsigned char*)plB + (int64_t)min(4 * Jb + p4, npB - 1) * kgs * 512 + within * 16;
    unsigned char* const wdst = lds + w * 1024;  // wave-uniform destination; the lanes land at + 16 lane
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < NW; ++s)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][s][i] = 0;

    const int nstage = kgs >> 2;
    gi_request_stage(gA, strideA, gB, strideB, wdst);
    if (nstage > 1) gi_request_stage(gA + 2048, strideA, gB + 2048, strideB, wdst + GI_STAGE_BYTES);
    int cur_off = 0, fill_off = 2 * GI_STAGE_BYTES;  // slot of stage st; slot of stage st + 2 = that of stage st - 1
    // lgkmcnt(0) with every wait: whatever the compiler moved, no operand read of the stage before is pending when this wave lets the others past
    // the barrier to overwrite that stage's slot
    for (int st = 0; st + 2 < nstage; ++st) {
        gA += 2048;
        gB += 2048;
        asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        gi_stage<NW, true>(lds + cur_off, lane, wi, wj, gA + 2048, strideA, gB + 2048, strideB, wdst + fill_off, acc);
        cur_off = cur_off == 2 * GI_STAGE_BYTES ? 0 : cur_off + GI_STAGE_BYTES;
        fill_off = fill_off == 2 * GI_STAGE_BYTES ? 0 : fill_off + GI_STAGE_BYTES;
    }
    if (nstage > 1) {  // the last stage but one: nothing left to request, the last stage stays in flight
        asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        gi_stage<NW, false>(lds + cur_off, lane, wi, wj, gA, strideA, gB, strideB, wdst, acc);
        cur_off = cur_off == 2 * GI_STAGE_BYTES ? 0 : cur_off + GI_STAGE_BYTES;
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    gi_stage<NW, false>(lds + cur_off, lane, wi, wj, gA, strideA, gB, strideB, wdst, acc);
}
