// svd_jacobi.hip — K4: batched economy SVD in fp32 by one-sided block Jacobi, written for gfx950.  HOST DRIVER (plans, launch sequences,
// convergence logic, C entry points); the device kernels are in jacobi_kernels.h / twolevel.h / tall_kernels.h (this translation unit) and
// evd_wave.hip (the 64x64 eigen-solves, their own translation unit).
//
// Replaces the factorisation at modules/svd_linear.py:65 (oracle: torch.linalg.svd, BASELINE.json) and the values-only torch.svd at
// sensitivity.py:101.  See DESIGN.md 3 for the algorithm and the roofline accounting.
//
// Data layout in HBM (per problem): the oriented matrix (rows >= cols) is stored as nb = ncols_pad/32 column panels.  Panel I is a dense
// [R][32] fp32 array (row stride 128 B = one cache line), so a wave reads two consecutive rows of a panel with ONE fully coalesced 256-B
// load, and a panel pair is two contiguous streams.  Rows [0, m_pad) hold A (times the column scale); rows [m_pad, m_pad + n_pad) exist
// only when the right vectors of a DIRECT call are wanted: the backsolve at the end writes them there (they are never rotated).
//
// A call:  [reduce: fp64 Gram + sorted Cholesky-QR, Jacobi then runs on R^T — svd_tall]  ->  sweeps (svd_direct_run)  ->  finalize.
// A dense sweep (two-level, twolevel.h): the internal step d = 1 with the single-level kernels, then per super-step TWO launches — evdw12
// (all 64x64 solves of the step) and supgram (update + next step's Gram tiles).  A sparse sweep: coupling snapshot, marked pairs packed into
// rounds of disjoint pairs, three single-level launches per round (gram_kernel, evdw0, update_kernel).
#include "common.h"
#include "jacobi_shared.h"
#include <vector>
#include <cmath>
#include <cstring>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstdarg>
#include <algorithm>
#include <type_traits>
#include <thread>
#include <mutex>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <fcntl.h>
#include <unistd.h>

namespace asvdk {
thread_local int g_call_cus = 0;   // see call_cus_now(): set per host thread for the duration of a half-batch call (0: the whole device)
// CUs of the current device (hipDeviceAttributeMultiprocessorCount, cached per device).  256 — the MI355X — when no device is visible: the
// host-side size queries (asvd_svd_worksize) answer on a CPU-only box too.
int device_cus() {
    static std::atomic<int> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    const int c = cache[dev].load(std::memory_order_relaxed);
    if (c > 0) return c;
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) return 256;
    cache[dev].store(ncu, std::memory_order_relaxed);
    return ncu;
}
int call_cus_now() { return g_call_cus > 0 ? g_call_cus : device_cus(); }
}
namespace {
using namespace asvdk;


#include "jacobi_kernels.h"
#include "tall_kernels.h"
#include "i8_digits.h"
#include "gram_i8.h"
#include "nn_gemm_i8.h"
#include "snapshot_i8.h"

struct Plan {
    int batch;
    int64_t m, n;         // as given
    int transposed;       // oriented = A^T when m < n
    int rows, cols;       // oriented dims, rows >= cols
    int m_pad, n_pad, nb, npairs, R, vmode;  // vmode: 0 no right vectors, 2 backsolve at the end (1, accumulate V in the sweeps, is gone)
    int nsplit, rows_per_split, rows_per_wg, nchunks;
    // two-level dense sweeps (twolevel.h): ns super-panels of 64 columns, npairs_s pair slots per super-step (power-of-two padded)
    int two, ns, npairs_s, nsplit_s, rows_per_split_s, nchunks_s, rows_per_wg_s, nchunks_q, rows_per_wg_q;
    size_t off_gd32, off_gx6, off_q0, off_d0, off_qfin, off_subact, off_din;
    int64_t panel_stride, batch_stride;
    // workspace offsets in bytes
    size_t off_x, off_xorig, off_gpart, off_q, off_active, off_sig, off_ina, off_inv, off_perm, off_flags, off_pflag, off_plist, off_snap, off_snapex, total;
};

constexpr int64_t MAX_DIM = 1 << 24;   // largest m and n of a call

int make_plan(int batch, int64_t m, int64_t n, int want_vv, Plan& p) {
    if (batch < 1 || m < 1 || n < 1 || m > MAX_DIM || n > MAX_DIM) return ASVD_E_BADARG;
    // CUs the launches of the current call may use: those of the device (256 on the MI355X), or those of one half when asvd_svd_batched runs a
    // batch as two halves on CU-masked streams (below).  The launch geometry of a plan (row splits, chunk counts) is sized for this many.
    const int64_t cu = call_cus_now();
    p.batch = batch;
    p.m = m;
    p.n = n;
    p.transposed = (m < n) ? 1 : 0;
    p.rows = (int)(p.transposed ? n : m);
    p.cols = (int)(p.transposed ? m : n);
    p.m_pad = (int)round_up64(p.rows, 32);
    p.n_pad = (int)round_up64(p.cols, PW);
    p.nb = p.n_pad / PB;
    {
        int pw2 = 2;
        while (pw2 < p.nb) pw2 <<= 1;
        p.npairs = pw2 / 2;  // XOR ordering runs over the panel count padded to a power of two
    }
    // want_vv: right vectors OF THE ORIENTED problem (backsolved V rows)
    p.vmode = want_vv ? 2 : 0;
    p.R = p.m_pad + (want_vv ? p.n_pad : 0);   // the V rows of a panel are written by the backsolve at the end, never rotated: updates cover m_pad rows
    // gram: choose the row split that minimises (rounds of resident workgroups) x (chunks per wave + fixed overhead).
    // 3 workgroups of 4 waves fit per CU (148 VGPR+AGPR) -> 768 slots; a grid of 1.3 x slots costs 2 full rounds.
    {
        const int64_t nchunk_total = p.m_pad / 32;
        int64_t best_ns = 1;
        double best_cost = 1e300;
        for (int64_t ns = 1; ns <= nchunk_total && ns <= 64; ++ns) {
            const int64_t wgs = ns * p.npairs * batch;
            const int64_t rounds = ceil_div64(wgs, 3 * cu);
            const int64_t chunks_wg = ceil_div64(nchunk_total, ns);
            const int64_t chunks_wave = ceil_div64(chunks_wg, 4);
            const double cost = (double)rounds * ((double)chunks_wave + 1.5) + 0.02 * ns;  // mild penalty: partials traffic
            if (cost < best_cost) { best_cost = cost; best_ns = ns; }
        }
        p.rows_per_split = (int)(ceil_div64(nchunk_total, best_ns) * 32);
        p.nsplit = (int)ceil_div64(p.m_pad, p.rows_per_split);
    }
    // update: 128-row iterations; aim for >= 1024 workgroups but >= 2 iterations per workgroup when possible
    int64_t wantc = ceil_div64(4 * cu, (int64_t)p.npairs * batch);
    int64_t iters_total = ceil_div64(p.m_pad, 128);
    int64_t nc = wantc < 1 ? 1 : (wantc > iters_total ? iters_total : wantc);
    p.rows_per_wg = (int)(ceil_div64(iters_total, nc) * 128);
    p.nchunks = (int)ceil_div64(p.m_pad, p.rows_per_wg);
    {
        // two-level dense sweeps for >= 8 panels; smaller problems run the single-level sweep
        p.two = p.nb >= 8 ? 1 : 0;
        p.ns = p.nb / 2;
        int pw2 = 2;
        while (pw2 < p.ns) pw2 <<= 1;
        p.npairs_s = pw2 / 2;
        // sgram6: 3 workgroups (32 KiB LDS, ~150 VGPRs) per CU -> 768 slots; 16-row chunks per wave, same cost model as the single-level Gram
        const int64_t nchunk_total = p.m_pad / 32;
        int64_t best_ns = 1;
        double best_cost = 1e300;
        for (int64_t ns = 1; ns <= nchunk_total && ns <= 64; ++ns) {
            const int64_t wgs = ns * p.npairs_s * batch;
            const int64_t rounds = ceil_div64(wgs, 3 * cu);
            const int64_t chunks_wave = ceil_div64(2 * ceil_div64(nchunk_total, ns), 4);
            const double cost = (double)rounds * ((double)chunks_wave + 1.5) + 0.02 * ns;
            if (cost < best_cost) { best_cost = cost; best_ns = ns; }
        }
        p.rows_per_split_s = (int)(ceil_div64(nchunk_total, best_ns) * 32);
        p.nsplit_s = (int)ceil_div64(p.m_pad, p.rows_per_split_s);
        // supdate: 32-row tiles; aim for >= 1024 workgroups per launch and >= 4 tiles per workgroup
        const int64_t tiles = ceil_div64(p.m_pad, 32);
        int64_t wantc = ceil_div64(4 * cu, (int64_t)p.npairs_s * batch);
        int64_t nc = std::max<int64_t>(1, std::min<int64_t>(wantc, ceil_div64(tiles, 4)));
        p.rows_per_wg_s = (int)(ceil_div64(tiles, nc) * 32);
        p.nchunks_s = (int)ceil_div64(p.m_pad, p.rows_per_wg_s);
        // supgram (update of a step fused with the Gram tiles of the next): one 512-thread workgroup per CU and quad of four
        // super-panels; ~512 workgroups per launch where the rows allow >= 8 tiles each
        // measured (16 x 4096^2): 2 chunks (512 workgroups) beat 4 and 8 — longer streams per workgroup, fewer partial tiles for the solves to sum
        const int64_t quads = std::max<int64_t>(1, pw2 / 4) * batch;
        // (and 1 chunk = exactly one workgroup per CU beats 2 once the quads alone fill the chip: 170.7 vs 174.0 ms per step, solves 97 vs 100)
        // small batches: one round of 256 workgroups too (batch 4: 43.7 ms of supgram per step with 4 chunks, 47.3 with 8, 52.8 with 16);
        // the solves sum the partial tiles with independent loads, so their cost no longer grows with the chunk count
        int64_t nq = std::max<int64_t>(1, std::min<int64_t>(ceil_div64(cu, quads), std::max<int64_t>(1, tiles / 8)));
        {
            // counts that are not a power of two (13B: 80 super-panels = 20 real quads per problem in a 32-quad grid): one workgroup per CU means
            // the launch runs in whole rounds of 256 workgroups, and 320 real workgroups cost two rounds (measured 1179 us per launch at
            // 16 x 5120^2; four row chunks = exactly five rounds of a quarter length: 737 us).  Pick the chunk count that wastes the least.
            const int64_t real = ceil_div64(p.ns, 4) * batch;
            if (real != quads && real >= cu) {
                double best = 1e300;
                for (int64_t c = 1; c <= 8 && c <= std::max<int64_t>(1, tiles / 8); c *= 2) {
                    const double cost = (double)ceil_div64(real * c, cu) / (double)c * (1.0 + 0.03 * (double)c);
                    if (cost < best) { best = cost; nq = c; }
                }
            }
        }
        p.rows_per_wg_q = (int)(ceil_div64(tiles, nq) * 32);
        p.nchunks_q = (int)ceil_div64(p.m_pad, p.rows_per_wg_q);
    }
    p.panel_stride = (int64_t)p.R * PB;
    p.batch_stride = p.panel_stride * p.nb;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    p.off_x = take((size_t)p.batch_stride * batch * sizeof(float));
    p.off_xorig = take(p.vmode == 2 ? (size_t)p.m_pad * PB * p.nb * batch * sizeof(float) : 0);
    p.off_gpart = take((size_t)batch * p.npairs * p.nsplit * 3072 * sizeof(float));
    p.off_q = take((size_t)batch * p.npairs * PW * PW * sizeof(float));
    p.off_active = take((size_t)batch * p.npairs * sizeof(int));
    p.off_sig = take((size_t)batch * p.n_pad * sizeof(float));
    p.off_ina = take((size_t)batch * p.n_pad * sizeof(float));
    p.off_inv = take((size_t)batch * p.n_pad * sizeof(float));
    p.off_perm = take((size_t)batch * p.n_pad * sizeof(int));
    p.off_flags = take((size_t)batch * 4 * sizeof(int));  // [maxoff bits | nrot | done | super-pair updates] x batch (SoA)
    p.off_pflag = take((size_t)batch * p.nb * p.nb);      // sparse-sweep pair marks
    p.off_plist = take((size_t)batch * p.nb * p.nb * sizeof(int));  // per-step lists of marked pairs (bound: steps x nb/2 slots per problem)
    // int8 digit planes + column exponents of the coupling snapshot (snapshot_i8.h): problems that can reach a sparse sweep and fit the int32 range
    const bool snap8 = p.nb >= 8 && p.m_pad <= 32768;
    p.off_snap = take(snap8 ? (size_t)3 * p.n_pad * round_up64(p.m_pad, 64) * batch : 0);
    p.off_snapex = take(snap8 ? (size_t)batch * p.n_pad * sizeof(int) : 0);
    const size_t t2 = p.two ? 1 : 0;
    p.off_gd32 = take(t2 * batch * p.nb * 1024 * sizeof(float));                          // carried 32x32 diagonal blocks, one per panel
    p.off_gx6 = take(t2 * batch * p.npairs_s * std::max(p.nsplit_s, p.nchunks_q) * 6 * 1024 * sizeof(float));  // sgram6 / supgram partial tiles
    p.off_q0 = take(t2 * batch * p.npairs_s * 2 * PW * PW * sizeof(float));               // Q of the two step-0 solves
    p.off_d0 = take(t2 * batch * p.npairs_s * 4 * 1024 * sizeof(float));                  // diagonal blocks after step 0
    p.off_qfin = take(t2 * batch * p.npairs_s * SP * SP * sizeof(float));                 // Q^(0) Q^(1) of every super-pair
    p.off_subact = take(t2 * batch * p.npairs_s * 4 * sizeof(int));
    p.off_din = take(t2 * batch * p.npairs_s * SP * sizeof(float));                        // pre-rotation squared column norms of every super-pair
    p.total = off;
    return ASVD_OK;
}

// grouped schedule (super_pair, super_order = 2): the group size G = 2^gb, 2 <= G <= 16, that divides ns into at most 16 groups with the fewest
// super-steps, G - 1 + G * rounds (rounds of a round-robin tournament over the groups: ng - 1 for an even group count, ng with a bye for an odd one);
// ties go to the larger group.  0: ns is a power of two, or nothing beats the padded XOR schedule.
static int group_bits_for(int ns) {
    if (ns < 4 || (ns & (ns - 1)) == 0) return 0;
    int pw2 = 2;
    while (pw2 < ns) pw2 <<= 1;
    int best = pw2 - 1, best_gb = 0;
    // groups of 16 first, as rounds 2-3 had them: with the 13B shapes' 80 super-panels the 95 steps of five groups of 16 (one with a bye per
    // round: 32 pairs per step = exactly one round of eigen-solve waves at batch 32) beat the 79 steps of ten groups of 8 (40 pairs per step,
    // one more dense sweep: 22.4 vs 27.1 SVD/s at 5120^2 x 32) — locality inside a group is worth more than a full schedule
    if (ns % 16 == 0 && ns / 16 <= 8 && 15 + 16 * (((ns / 16) & 1) ? ns / 16 : ns / 16 - 1) < pw2 - 1) return 4;
    for (int gb = 4; gb >= 1; --gb) {
        const int G = 1 << gb;
        if (ns % G) continue;
        const int ng = ns / G;
        if (ng < 2 || ng > 16) continue;
        const int steps = G - 1 + G * ((ng & 1) ? ng : ng - 1);
        if (steps < best) { best = steps; best_gb = gb; }
    }
    return best_gb;
}
static int grouped_rounds(int ns, int gb) { const int ng = ns >> gb; return (ng & 1) ? ng : ng - 1; }
static int grouped_steps(int ns, int gb) { return (1 << gb) - 1 + (1 << gb) * grouped_rounds(ns, gb); }
// group pairs of every round: circle method over the ns / G groups (+ a bye when their number is odd)
static void set_group_table(Sched& sc, int ns, int gb) {
    const int ng = ns >> gb, n = ng + (ng & 1), gm = ng / 2;
    signed char (*tab)[8][2] = sc.gpair;
    std::memset(sc.gpair, 0, sizeof(sc.gpair));
    for (int r = 0; r < n - 1; ++r) {
        int m = 0;
        for (int k = 0; k < n / 2; ++k) {
            const int a = (k == 0) ? 0 : 1 + (k - 1 + r) % (n - 1);
            const int pb = n - 1 - k;
            const int bb = 1 + (pb - 1 + r) % (n - 1);
            if (a >= ng || bb >= ng) continue;  // the bye
            tab[r][m][0] = (signed char)std::min(a, bb);
            tab[r][m][1] = (signed char)std::max(a, bb);
            ++m;
        }
    }
    sc.gm = gm;
    sc.gb = gb;
}
static bool grouped_applies(int ns) { return group_bits_for(ns) > 0; }
static bool super_grouped_for(const Plan& p) {
    return p.two && grouped_applies(p.ns);
}

// test hook asvd_test_super_schedule: slot k of super-step `step` of the super-panel pair schedule
__global__ void super_schedule_kernel(Sched sc, int ns, int nsteps, int npairs, int* __restrict__ out) {
    const int step = blockIdx.x, k = threadIdx.x;
    if (k >= npairs) return;
    int S, T;
    super_pair(sc, ns, step, k, S, T);
    out[step * npairs + k] = (S < ns && T < ns) ? ((S << 16) | T) : -1;
}

// test hook asvd_test_i8_tile: gi_tile_loop alone (i8_digits.h), the raw accumulators of every 128 x 128 block of two plane sets, out[s][32 npA][32 npB] (int32).  grid (ceil(npB / 4), ceil(npA / 4)).
template <int NW>
__global__ __launch_bounds__(512) void i8_tile_test_kernel(const signed char* __restrict__ plA, int64_t strideA, int npA, const signed char* __restrict__ plB,
                                                           int64_t strideB, int npB, int kgs, int* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gi_lds[];  // GI_LDS_BYTES
    const int Ib = blockIdx.y, Jb = blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wi = w >> 2, wj = w & 3;
    i32x16 acc[2][NW];
    gi_tile_loop<NW>(plA, strideA, npA, plB, strideB, npB, Ib, Jb, kgs, gi_lds, acc);
    const int J = 4 * Jb + wj;
    if (J >= npB) return;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int I = 4 * Ib + 2 * wi + t;
        if (I >= npA) continue;
#pragma unroll
        for (int s = 0; s < NW; ++s)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int i = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
                out[((int64_t)s * 32 * npA + I * 32 + i) * (32 * npB) + J * 32 + (lane & 31)] = acc[t][s][reg];
            }
    }
}

// what svd_tall and the split of a batch return when they do not apply: the caller then runs the plain call
constexpr int NOT_APPLICABLE = -100;   // the reduction (Cholesky breakdown, workspace too small for it), or the split (workspace, sizes)
constexpr int SPLIT_REFUSED = -101;    // the split: refused (another process on the device, a CU-masked caller stream, no CU-masked streams)

// ASVD_DEBUG: one line of the driver's trace on stderr
__attribute__((format(printf, 1, 2))) static void debug_trace(const char* fmt, ...) {
    if (!getenv("ASVD_DEBUG")) return;
    char line[512];
    va_list ap;
    va_start(ap, fmt); vsnprintf(line, sizeof(line), fmt, ap); va_end(ap);
    fprintf(stderr, "[asvd_svd] %s\n", line);
}
static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// ---- optional per-class timing with HIP events on the call's stream ------------------------------
// classes: 0 pack / reduce, 1 two-level Gram pass, 2 eigen-solves, 3 two-level update pass, 4 finalize, 5 coupling snapshot,
//          6 single-level Gram, 7 single-level update, 8 fused two-level update + Gram pass
constexpr int NPROF = 9;
struct ProfRec { int cls; hipEvent_t a, b; };
// What the profiled calls of ONE host thread measured: concurrent calls from different threads (on their own streams and workspaces) do not
// share it.  The second half of a split call fills the record of the worker thread, which hands the whole record back to the caller.
struct Profile {
    bool on = false;                           // asvd_svd_set_profiling
    float ms[NPROF] = {};
    int launches[NPROF] = {};
    long long pairs[3] = {};                   // 32-panel pair visits, rotated 32-panel pairs, updated super-pairs (two-level sweeps)
    std::vector<float> sweep_ms;               // wall time of every sweep of the last profiled call (all problems of the batch together)
    std::vector<long long> sweep_rot;          // pairs rotated in it
    std::vector<ProfRec> recs;                 // event pairs not yet read
    std::vector<std::pair<float, float>> iv8;  // [start, end] of every class-8 launch, ms after the base event given to end()
    void begin() { *this = Profile{on}; }
    // base: an event recorded before the call started (split mode, below), or nullptr: no class-8 intervals
    void end(hipEvent_t base) {
        for (auto& r : recs) {
            float t = 0;
            (void)hipEventSynchronize(r.b);
            (void)hipEventElapsedTime(&t, r.a, r.b);
            ms[r.cls] += t;
            launches[r.cls] += 1;
            if (r.cls == 8 && base) {
                float t0 = 0;
                if (hipEventElapsedTime(&t0, base, r.a) == hipSuccess) iv8.emplace_back(t0, t0 + t);
            }
            (void)hipEventDestroy(r.a);
            (void)hipEventDestroy(r.b);
        }
        recs.clear();
    }
    void add(const Profile& o) {
        for (int i = 0; i < NPROF; ++i) { ms[i] += o.ms[i]; launches[i] += o.launches[i]; }
        for (int i = 0; i < 3; ++i) pairs[i] += o.pairs[i];
    }
};
thread_local Profile g_prof;
thread_local bool g_prof_keep_split = false;   // asvd_svd_set_profiling(2): a profiled call keeps the split (else it runs UNSPLIT: every kernel alone on the chip)
// The split-mode profile (mode 2): both halves time their own launches with events on their own stream, and the [start, end] of every fused
// update + Gram launch (class 8) of both halves is placed on ONE time axis — the union / overlap of the two halves' HBM-bound launches is what
// the combined streaming rate of a split step follows from.
struct SplitProfile {
    bool last = false;   // the last asvd_svd_batched call of this thread ran split
    float ms[2][NPROF] = {};
    int launches[2][NPROF] = {};
    float overlap[4] = {};   // class 8: summed ms of half 0, of half 1, union of both, time BOTH were in it
};
thread_local SplitProfile g_split_prof;
// which path the last asvd_svd_batched call of this host thread took (asvd_svd_get_last_path): ASVD_PATH_* bits of include/asvd_hip.h
thread_local int g_last_path = 0;

// class-8 intervals of both halves on one time axis -> SplitProfile::overlap
static void class8_overlap(const std::vector<std::pair<float, float>>& iv0, const std::vector<std::pair<float, float>>& iv1, float out[4]) {
    std::vector<std::pair<float, int>> edges;
    float sum[2] = {0, 0};
    for (int h = 0; h < 2; ++h)
        for (auto& iv : h ? iv1 : iv0) { edges.emplace_back(iv.first, +1); edges.emplace_back(iv.second, -1); sum[h] += iv.second - iv.first; }
    std::sort(edges.begin(), edges.end());
    float uni = 0, both = 0, last = 0;
    int depth = 0;
    for (auto& e : edges) {
        if (depth >= 1) uni += e.first - last;
        if (depth >= 2) both += e.first - last;
        last = e.first;
        depth += e.second;
    }
    out[0] = sum[0]; out[1] = sum[1]; out[2] = uni; out[3] = both;
}

struct ProfScope {
    int cls; hipStream_t st; hipEvent_t a = nullptr, b = nullptr; bool on;
    ProfScope(int c, hipStream_t s) : cls(c), st(s), on(g_prof.on) {
        if (on) { (void)hipEventCreate(&a); (void)hipEventCreate(&b); (void)hipEventRecord(a, st); }
    }
    ~ProfScope() {
        if (on) { (void)hipEventRecord(b, st); g_prof.recs.push_back({cls, a, b}); }
    }
};

template <int DT>
int launch_pack(const void* src, int64_t ld, const void* s, int cs_dtype, const Plan& p, float* Xb, hipStream_t st) {
    dim3 grid((unsigned)ceil_div64(p.rows, 32), (unsigned)ceil_div64(p.cols, 256));
    const int has = s ? 1 : 0;
    switch (cs_dtype) {
        case ASVD_F32: pack_kernel<DT, ASVD_F32><<<grid, 256, 0, st>>>(src, ld, s, has, p.transposed, p.rows, p.cols, p.R, Xb); break;
        case ASVD_F16: pack_kernel<DT, ASVD_F16><<<grid, 256, 0, st>>>(src, ld, s, has, p.transposed, p.rows, p.cols, p.R, Xb); break;
        case ASVD_BF16: pack_kernel<DT, ASVD_BF16><<<grid, 256, 0, st>>>(src, ld, s, has, p.transposed, p.rows, p.cols, p.R, Xb); break;
        default: return ASVD_E_BADARG;
    }
    return ASVD_OK;
}

// every problem of the batch into its panels (p.batch_stride floats per problem from X on)
int pack_batch(const void* const* a_host, int a_dtype, int64_t lda, const void* const* cs_host, int cs_dtype, const Plan& p, float* X, hipStream_t st) {
    for (int b = 0; b < p.batch; ++b) {
        float* Xb = X + (int64_t)b * p.batch_stride;
        const void* s = cs_host ? cs_host[b] : nullptr;
        int prc;
        switch (a_dtype) {
            case ASVD_F32: prc = launch_pack<ASVD_F32>(a_host[b], lda, s, cs_dtype, p, Xb, st); break;
            case ASVD_F16: prc = launch_pack<ASVD_F16>(a_host[b], lda, s, cs_dtype, p, Xb, st); break;
            default: prc = launch_pack<ASVD_BF16>(a_host[b], lda, s, cs_dtype, p, Xb, st); break;
        }
        if (prc) return prc;
    }
    return ASVD_OK;
}

// Sparse sweeps: marks -> lists of disjoint pairs.  The pairs of one XOR step (I ^ J == d) are disjoint by construction, but late in the
// iteration a step holds a handful of pairs and a sweep of nb-1 three-launch steps is all launch latency.  The marked pairs of every running
// problem (flags: [batch][nb][nb], host_done: [batch]) are therefore packed first-fit, in schedule order (step, then I), into at most nsteps
// ROUNDS whose pairs share no panel (per problem: a bitmask of used panels per round); a round is launched like a step.  Any order of disjoint
// rotations is a valid Jacobi sweep; first-fit keeps the nearest-neighbour-first order of the XOR schedule among conflicting pairs.
// list: cnt[r] slots per problem for round r from off[r] on (code I << 16 | J, -1 = empty slot).  Returns the number of marked pairs.
static long long pack_marked_pairs(const std::vector<unsigned char>& flags, const std::vector<int>& host_done, int nb, int nsteps,
                                   std::vector<int>& list, std::vector<int>& off, std::vector<int>& cnt) {
    const int batch = (int)host_done.size();
    long long marked_total = 0;
    list.clear();
    std::vector<std::vector<int>> tmp((size_t)batch * nsteps);  // [b * nsteps + round]
    const int words = (nb + 63) / 64;
    std::vector<uint64_t> used;  // [round][words] of the problem being packed
    for (int b = 0; b < batch; ++b) {
        if (host_done[b]) continue;
        const unsigned char* f = flags.data() + (size_t)b * nb * nb;
        bool packed = true;
        used.assign((size_t)nsteps * words, 0);
        long long n = 0;
        for (int d = 1; d <= nsteps && packed; ++d)
            for (int I = 0; I < nb && packed; ++I) {
                const int J = I ^ d;
                if (J <= I || J >= nb || !f[(size_t)I * nb + J]) continue;
                int r = 0;
                for (; r < nsteps; ++r) {
                    uint64_t* u = &used[(size_t)r * words];
                    if (!((u[I >> 6] >> (I & 63)) & 1) && !((u[J >> 6] >> (J & 63)) & 1)) {
                        u[I >> 6] |= 1ull << (I & 63);
                        u[J >> 6] |= 1ull << (J & 63);
                        break;
                    }
                }
                if (r == nsteps) { packed = false; break; }  // cannot happen below ~nsteps/2 marks per panel; fall back
                tmp[(size_t)b * nsteps + r].push_back((I << 16) | J);
                ++n;
            }
        if (packed) marked_total += n;
        else {  // one list per XOR step
            for (int r = 0; r < nsteps; ++r) tmp[(size_t)b * nsteps + r].clear();
            for (int I = 0; I < nb; ++I)
                for (int J = I + 1; J < nb; ++J)
                    if (f[(size_t)I * nb + J]) { tmp[(size_t)b * nsteps + ((I ^ J) - 1)].push_back((I << 16) | J); ++marked_total; }
        }
    }
    for (int r = 0; r < nsteps; ++r) {
        size_t mx = 0;
        for (int b = 0; b < batch; ++b) mx = std::max(mx, tmp[(size_t)b * nsteps + r].size());
        cnt[r] = (int)mx;
        off[r] = (int)list.size();
        for (int b = 0; b < batch; ++b) {
            const auto& v = tmp[(size_t)b * nsteps + r];
            for (size_t i = 0; i < mx; ++i) list.push_back(i < v.size() ? v[i] : -1);
        }
    }
    return marked_total;
}

// ---- the direct driver: sweeps on the packed panels, then finalize ----------------------------------------------------------------------
// The fixed state of one call: its plan, the workspace as the kernels see it, the schedule and the stream.
struct Direct {
    Plan p;
    hipStream_t st;
    char* wb;
    float *X, *Gpart, *Qbuf, *sig, *ina, *inv;
    int *active, *perm, *nrot, *done, *nupd, *plist;
    unsigned* maxoff;
    unsigned char* pflag;   // sparse-sweep pair marks (see fullcheck_kernel)
    Sched sc;               // the call's schedule description: a kernel argument of every launch (no process-global device state)
    EvdV3 v3;               // buffers of the two-level sweeps as the kernels see them
    int kb;                 // panels whose convergence is enforced: those holding the k leading columns, plus one panel of margin
    int nsteps;             // steps of a single-level sweep (XOR distances 1 .. nsteps)
    float tol;
};
// one inner sweep of the 64x64 eigen-solve per visit: with the XOR schedule a second one no longer saves outer sweeps
// (measured 26.3 vs 25.9 SVD/s)
constexpr int inner_sweeps = 1;

static void direct_bind(Direct& c, void* work, hipStream_t st, int64_t k, float tol) {
    const Plan& p = c.p;
    char* wb = (char*)work;
    c.st = st;
    c.wb = wb;
    c.X = (float*)(wb + p.off_x); c.Gpart = (float*)(wb + p.off_gpart); c.Qbuf = (float*)(wb + p.off_q); c.active = (int*)(wb + p.off_active);
    c.sig = (float*)(wb + p.off_sig); c.ina = (float*)(wb + p.off_ina); c.inv = (float*)(wb + p.off_inv); c.perm = (int*)(wb + p.off_perm);
    // flags: [maxoff bits | nrot | done | super-pair updates (instrumentation)] x batch (SoA)
    c.maxoff = (unsigned*)(wb + p.off_flags);
    c.nrot = (int*)(wb + p.off_flags) + p.batch;
    c.done = (int*)(wb + p.off_flags) + 2 * p.batch;
    c.nupd = (int*)(wb + p.off_flags) + 3 * p.batch;
    c.pflag = (unsigned char*)(wb + p.off_pflag);
    c.plist = (int*)(wb + p.off_plist);
    c.sc = default_sched();
    c.sc.super_order = super_grouped_for(p) ? 2 : 1;
    if (c.sc.super_order == 2) set_group_table(c.sc, p.ns, group_bits_for(p.ns));
    c.v3 = EvdV3{};
    c.v3.ns = p.ns;
    c.v3.nbpan = p.nb;
    c.v3.Gd32 = (float*)(wb + p.off_gd32); c.v3.Q0 = (float*)(wb + p.off_q0); c.v3.D0 = (float*)(wb + p.off_d0);
    c.v3.Qfin = (float*)(wb + p.off_qfin); c.v3.subact = (int*)(wb + p.off_subact); c.v3.Din = (float*)(wb + p.off_din);
    c.kb = (int)(ceil_div64(k, PB) + 1 < p.nb ? ceil_div64(k, PB) + 1 : p.nb);
    c.nsteps = 2 * p.npairs - 1;
    c.tol = tol;
}

static int direct_pack(const Direct& c, const void* const* a_host, int a_dtype, int64_t lda, const void* const* cs_host, int cs_dtype) {
    const Plan& p = c.p;
    ProfScope ps(0, c.st);
    ASVD_HIP_CHECK(hipMemsetAsync(c.X, 0, (size_t)p.batch_stride * p.batch * sizeof(float), c.st));
    ASVD_HIP_CHECK(hipMemsetAsync(c.wb + p.off_flags, 0, (size_t)p.batch * 4 * sizeof(int), c.st));
    if (int prc = pack_batch(a_host, a_dtype, lda, cs_host, cs_dtype, p, c.X, c.st)) return prc;
    if (p.vmode == 2) {
        // keep the packed original (A rows of every panel) for the final backsolve
        ASVD_HIP_CHECK(hipMemcpy2DAsync(c.wb + p.off_xorig, (size_t)p.m_pad * PB * sizeof(float), c.X, (size_t)p.R * PB * sizeof(float),
                                        (size_t)p.m_pad * PB * sizeof(float), (size_t)p.nb * p.batch, hipMemcpyDeviceToDevice, c.st));
    }
    return ASVD_OK;
}

// Step schedule of a single-level dense sweep (XOR distances d, stored as step = d-1).  The local levels d = 1..L are run twice at the
// start of every sweep: the strongest couplings of the sorted, preconditioned matrix sit between neighbouring panels, and a second pass
// over them is cheap (L extra steps of P-1) — docs/history.md (round 1).  L = min(7, P/16 - 1): measured at 4096^2 (P = 128) 8 -> 7 sweeps, +2.4 %.
static std::vector<int> single_level_schedule(int nsteps) {
    std::vector<int> sched;
    const int P2 = nsteps + 1;
    const int L = std::min(std::max(0, std::min(7, P2 / 16 - 1)), nsteps);
    for (int d = 1; d <= L; ++d) sched.push_back(d - 1);
    for (int st2 = 0; st2 < nsteps; ++st2) sched.push_back(st2);
    return sched;
}

// marks of the coupling snapshot (host copy) and the rounds of disjoint pairs packed from them (pack_marked_pairs)
struct SparseLists { std::vector<unsigned char> marks; std::vector<int> list, off, cnt; };

// Opens a sparse sweep: snapshot of all couplings, marks read back, packed into rounds of disjoint pairs, the lists uploaded.
static int sparse_snapshot(const Direct& c, const std::vector<int>& host_done, SparseLists& sl, long long* marked,
                           std::chrono::steady_clock::time_point t0) {
    const Plan& p = c.p; const int batch = p.batch; const hipStream_t st = c.st;
    float* dnorm = c.ina;  // squared column norms of the snapshot (finalize overwrites this buffer later)
    {
        ProfScope ps(5, st);
        ASVD_HIP_CHECK(hipMemsetAsync(c.pflag, 0, (size_t)batch * p.nb * p.nb, st));
        const unsigned nt = (unsigned)ceil_div64(p.nb, 4);
        const char* es8 = getenv("ASVD_SNAP_I8");   // read per call
        const bool snap8 = p.nb >= 8 && p.m_pad <= 32768 && !(es8 && atoi(es8) == 0);
        if (snap8) panel_sumsq_max_kernel<<<dim3(p.nb, batch), 256, 0, st>>>(c.X, p.panel_stride, p.batch_stride, p.m_pad, p.n_pad, dnorm, (int*)(c.wb + p.off_snapex), c.done);
        else panel_sumsq_kernel<<<dim3(p.nb, batch), 256, 0, st>>>(c.sc, c.X, p.panel_stride, p.batch_stride, p.m_pad, p.n_pad, dnorm, c.done);
        if (snap8) {
            // X^T X from int8 digit planes (snapshot_i8.h): digitise once, eight exact digit products per fp32 product
            int* sex = (int*)(c.wb + p.off_snapex);
            signed char* spl = (signed char*)(c.wb + p.off_snap);
            const int kgs = (int)(round_up64(p.m_pad, 64) / 16);
            const int64_t plane_stride = (int64_t)p.nb * kgs * 512;
            split_i8_kernel<<<dim3(p.nb, (unsigned)ceil_div64(kgs, 8), batch), 256, 0, st>>>(c.X, p.panel_stride, p.batch_stride, p.nb, p.m_pad, p.n_pad, sex, 0,
                                                                                           kgs, spl, plane_stride, nullptr, c.done);
            ASVD_HIP_CHECK(hipFuncSetAttribute((const void*)fullcheck_i8_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, GI_LDS_BYTES));
            fullcheck_i8_kernel<<<dim3(nt * (nt + 1) / 2, batch), 512, GI_LDS_BYTES, st>>>(spl, plane_stride, p.nb, kgs, p.n_pad, sex, dnorm, c.tol, c.kb,
                                                                                              c.pflag, c.maxoff, c.done, (int)nt);
        } else {
            fullcheck_kernel<<<dim3(nt, nt, batch), 256, 0, st>>>(c.sc, c.X, p.panel_stride, p.batch_stride, p.nb, p.m_pad, p.n_pad, dnorm, c.tol, c.kb, c.pflag,
                                                                  c.maxoff, c.done);
        }
    }
    sl.marks.resize((size_t)batch * p.nb * p.nb);
    ASVD_HIP_CHECK(hipMemcpyAsync(sl.marks.data(), c.pflag, sl.marks.size(), hipMemcpyDeviceToHost, st));
    ASVD_HIP_CHECK(hipStreamSynchronize(st));
    debug_trace("  snapshot + readback %.2f ms", ms_since(t0));
    sl.off.resize(c.nsteps);
    sl.cnt.resize(c.nsteps);
    *marked = pack_marked_pairs(sl.marks, host_done, p.nb, c.nsteps, sl.list, sl.off, sl.cnt);
    debug_trace("  lists built at %.2f ms (%zu slots)", ms_since(t0), sl.list.size());
    if (!sl.list.empty()) ASVD_HIP_CHECK(hipMemcpyAsync(c.plist, sl.list.data(), sl.list.size() * sizeof(int), hipMemcpyHostToDevice, st));
    return ASVD_OK;
}

// The rounds of a sparse sweep, three single-level launches each.
static void sparse_rounds(const Direct& c, const SparseLists& sl) {
    const Plan& p = c.p; const int batch = p.batch; const hipStream_t st = c.st;
    for (int step = 0; step < c.nsteps; ++step) {
        const int slots = sl.cnt[step];
        if (slots == 0) continue;  // no marked pair meets in this round
        const int* pl = c.plist + sl.off[step];
        // few pairs per launch: split the rows further to fill the CUs, within the partial-Gram capacity of a problem
        const int64_t chunks = p.m_pad / 32, cap = (int64_t)p.npairs * p.nsplit / slots;
        int64_t ns = std::max<int64_t>(p.nsplit, ceil_div64(3 * call_cus_now(), (int64_t)slots * batch));
        ns = std::min<int64_t>(std::min<int64_t>(ns, cap), std::min<int64_t>(chunks, 64));
        if (ns < 1) ns = 1;
        const int rps = (int)(ceil_div64(chunks, ns) * 32);
        const int nsp = (int)ceil_div64(p.m_pad, rps);
        const int64_t iters = ceil_div64(p.m_pad, 128);
        int64_t nc = std::min<int64_t>(iters, std::max<int64_t>(1, ceil_div64(4 * call_cus_now(), (int64_t)slots * batch)));
        const int rpw = (int)(ceil_div64(iters, nc) * 128);
        const int nch = (int)ceil_div64(p.m_pad, rpw);
        {
            ProfScope ps(6, st);
            gram_kernel<<<dim3(nsp, slots, batch), 256, 0, st>>>(c.sc, c.X, p.panel_stride, p.batch_stride, p.nb, step, p.m_pad, rps, c.Gpart, c.done, pl, slots);
        }
        {
            ProfScope ps(2, st);
            launch_evdw0(false, slots, batch, st, c.sc, c.Gpart, nsp, c.Qbuf, c.active, c.maxoff, c.nrot, c.done, c.tol, inner_sweeps, p.nb, step, c.kb, pl, slots, EvdV3{});
        }
        {
            ProfScope ps(7, st);
            update_kernel<<<dim3(nch, slots, batch), 256, 0, st>>>(c.sc, c.X, p.panel_stride, p.batch_stride, p.nb, step, p.m_pad, rpw, c.Qbuf, c.active, c.done, pl, slots);
        }
    }
}

// Dense single-level steps, three launches each.  carry: the internal step of a two-level sweep, whose eigen-solves also emit the fresh
// carried diagonal blocks of both panels of every pair.
static void single_level_steps(const Direct& c, const std::vector<int>& steps, bool carry) {
    const Plan& p = c.p; const int batch = p.batch; const hipStream_t st = c.st;
    for (const int step : steps) {
        {
            ProfScope ps(6, st);
            gram_kernel<<<dim3(p.nsplit, p.npairs, batch), 256, 0, st>>>(c.sc, c.X, p.panel_stride, p.batch_stride, p.nb, step, p.m_pad, p.rows_per_split, c.Gpart,
                                                                      c.done, nullptr, 0);
        }
        {
            ProfScope ps(2, st);
            launch_evdw0(carry, p.npairs, batch, st, c.sc, c.Gpart, p.nsplit, c.Qbuf, c.active, c.maxoff, c.nrot, c.done, c.tol, inner_sweeps, p.nb, step, c.kb,
                         nullptr, 0, carry ? c.v3 : EvdV3{});
        }
        {
            ProfScope ps(7, st);
            update_kernel<<<dim3(p.nchunks, p.npairs, batch), 256, 0, st>>>(c.sc, c.X, p.panel_stride, p.batch_stride, p.nb, step, p.m_pad, p.rows_per_wg, c.Qbuf,
                                                                         c.active, c.done, nullptr, 0);
        }
    }
}

// The super-steps of a two-level dense sweep, two or three launches each.  *fused_used: the fused update + Gram kernel ran.
static int super_steps(Direct& c, bool allow_f16, bool* fused_used) {
    const Plan& p = c.p; const int batch = p.batch; const hipStream_t st = c.st;
    float* Gx6 = (float*)(c.wb + p.off_gx6);
    const bool super_grp = super_grouped_for(p);
    const int sgb = super_grp ? group_bits_for(p.ns) : 0, sG1 = (1 << sgb) - 1;   // grouped schedule: group size - 1
    const int nsuper = super_grp ? grouped_steps(p.ns, sgb) : 2 * p.npairs_s - 1;
    // supgram: the update of step D also leaves the Gram tiles of the step that follows (one pass instead of two); the stand-alone Gram
    // pass then runs only in front of the first super-step.  ASVD_SUPGRAM=0 keeps the separate passes (fp32 Gram pass, split-bf16 update
    // pass: also what a call falls back to when the split-fp16 path of the fused kernel turns a problem NaN).
    const bool fuse_ug = allow_f16 && p.npairs_s >= 2 && !(getenv("ASVD_SUPGRAM") && atoi(getenv("ASVD_SUPGRAM")) == 0);
    *fused_used = *fused_used || fuse_ug;
    if (fuse_ug)
        ASVD_HIP_CHECK(hipFuncSetAttribute((const void*)supgram_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(SUPGRAM_SMEM_FLOATS * sizeof(float))));
    // on a padded XOR schedule (ns not a power of two and no grouped schedule) many super-steps hold few real pairs and the fused kernel,
    // which reads every panel of a quad with a present member, loses to the separate passes, which touch only the pairs that exist
    // (13B shapes, ns = 80 in a 128-wide schedule: always fused 21.4 s, never fused 16.9 s for the model): fused on full schedules only
    const bool ns_pow2 = (p.ns & (p.ns - 1)) == 0;
    // (Round 5 measured a LINE-SPREAD order of the distances from a given dense sweep on — triples {d, w(d), w^2(d)} that close the four
    // super-panels of a quad — against this one: slower from every starting sweep, profiles/r5_spread_order_from_sweep.txt; removed.)
    auto fused_after = [&](int dj) {  // does the launch of super-step index dj also leave the tiles of index dj + 1 ?
        if (!fuse_ug || dj < 0 || dj + 1 >= nsuper) return false;
        if (super_grp) {  // consecutive steps inside the groups (XOR distances 1..15), or consecutive offsets of the same round of group pairs
            const int s0 = dj, s1 = dj + 1;   // 0-based super-steps
            return s1 < sG1 || (s0 >= sG1 && ((s0 - sG1) >> sgb) == ((s1 - sG1) >> sgb));
        }
        return ns_pow2;
    };
    EvdV3& v3 = c.v3;
    for (int di = 0; di < nsuper; ++di) {
        const int D = di + 1;
        const int E = (di + 1 < nsuper) ? di + 2 : 0;  // 0: last super-step of the sweep
        const bool gram_in = !fused_after(di - 1);   // tiles of this step not left by the previous launch
        const bool gram_out = fused_after(di);
        v3.nsplit6 = gram_in ? p.nsplit_s : p.nchunks_q;
        v3.Gx6 = Gx6;
        if (gram_in) {
            ProfScope ps(1, st);
            sgram6_kernel<<<dim3(p.nsplit_s, p.npairs_s, batch), 256, 0, st>>>(c.sc, c.X, p.panel_stride, p.batch_stride, p.ns, D, p.m_pad, p.rows_per_split_s, Gx6, c.done);
        }
        {
            ProfScope ps(2, st);  // both inner steps of every super-pair in one launch, one wave per 64x64 solve (evd_wave.hip)
            launch_evdw12(p.npairs_s, batch, st, c.sc, c.maxoff, c.nrot, c.done, c.tol, inner_sweeps, p.nb, D - 1, c.kb, v3, p.cols >= 2048);
        }
        {
            ProfScope ps(gram_out ? 8 : 3, st);
            if (gram_out)
                supgram_kernel<<<dim3(p.nchunks_q, (2 * p.npairs_s) / 4, batch), 512, SUPGRAM_SMEM_FLOATS * sizeof(float), st>>>(
                    c.sc, c.X, p.panel_stride, p.batch_stride, p.ns, D, E, p.m_pad, p.m_pad, p.rows_per_wg_q, v3.Qfin, v3.subact, v3.Din, Gx6, c.done, c.nupd, p.npairs_s);
            else
                supdate_split_kernel<<<dim3(p.nchunks_s, p.npairs_s, batch), 256, 0, st>>>(c.sc, c.X, p.panel_stride, p.batch_stride, p.ns, D, p.m_pad,
                                                                                        p.rows_per_wg_s, v3.Qfin, v3.subact, c.done, c.nupd);
        }
    }
    return ASVD_OK;
}

// per-problem state of the sweeps: what info_host reports; done mirrors the device's done flags
struct Progress {
    std::vector<int> status, sweeps, last_rot, done;
    std::vector<float> last_off, prev_off;
    explicit Progress(int batch)
        : status(batch, ASVD_N_NOCONV), sweeps(batch, 0), last_rot(batch, 0), done(batch, 0), last_off(batch, 0.0f), prev_off(batch, 1e30f) {}
};

// Profile and ASVD_DEBUG record of the sweep just done, over the problems that were still running in it.
// flags: [maxoff bits | nrot | done | super-pair updates] x batch, as read back after the sweep.
static void note_sweep(const Plan& p, const Progress& pr, const std::vector<int>& flags, int sweep, bool sparse, long long marked, double ms) {
    const int batch = p.batch;
    long long rot = 0, upd = 0, running = 0;
    for (int b = 0; b < batch; ++b)
        if (!pr.done[b]) { rot += flags[batch + b]; upd += flags[3 * batch + b]; ++running; }
    if (g_prof.on) {
        g_prof.sweep_ms.push_back((float)ms);
        g_prof.sweep_rot.push_back(rot);
        g_prof.pairs[0] += sparse ? marked : running * ((long long)p.nb * (p.nb - 1) / 2);
        g_prof.pairs[1] += rot;
        g_prof.pairs[2] += upd;
    }
    debug_trace("sweep %d%s wall %.2f ms, rotated pairs (all problems) %lld, marked %lld", sweep + 1, sparse ? " (sparse)" : "", ms, rot, marked);
}

// The convergence rules, per problem still running, from the flags of the sweep just done.  Returns true when every problem has finished;
// *changed: a problem finished in this sweep.
static bool update_convergence(Progress& pr, const std::vector<int>& flags, int sweep, float tol, bool* changed) {
    const int batch = (int)pr.done.size();
    bool all_done = true;
    for (int b = 0; b < batch; ++b) {
        if (pr.done[b]) continue;
        float mo;
        const unsigned bits = (unsigned)flags[b];
        std::memcpy(&mo, &bits, sizeof(float));
        pr.sweeps[b] = sweep + 1;
        pr.last_rot[b] = flags[batch + b];
        pr.last_off[b] = mo;
        debug_trace("b=%d sweep=%d maxoff=%.3e rotated_pairs=%d", b, sweep + 1, mo, pr.last_rot[b]);
        bool finished = true;
        if (mo != mo) pr.status[b] = ASVD_N_NAN;
        // Jacobi converges quadratically: a sweep that STARTED with max |cos| = mo leaves ~mo^2 behind, so a sweep with
        // mo < 0.3 sqrt(tol) has already produced orthogonality below tol (pairs above tol were all rotated in it).
        else if (mo < tol || mo < 0.3f * sqrtf(tol)) pr.status[b] = ASVD_OK;
        // stagnation at the fp32 noise floor: the scaled off-diagonal stopped contracting well below the level that
        // matters for the 1e-4 sigma / 1e-3 reconstruction contract (second-order in maxoff) -> converged
        else if (mo < 100.0f * tol && mo > 0.25f * pr.prev_off[b]) pr.status[b] = ASVD_OK;
        else finished = all_done = false;
        if (finished) { pr.done[b] = 1; *changed = true; }
        pr.prev_off[b] = mo;
    }
    return all_done;
}

// the next sweep is sparse once fewer than half of the pairs of the still-running problems rotated in this one
static bool next_sweep_sparse(const Plan& p, const Progress& pr) {
    if (p.nb < 8) return false;
    long long rot = 0, tot = 0;
    for (int b = 0; b < p.batch; ++b)
        if (!pr.done[b]) { rot += pr.last_rot[b]; tot += (long long)p.nb * (p.nb - 1) / 2; }
    return tot > 0 && (double)rot < 0.5 * (double)tot;
}

// Backsolve (right vectors), column norms, ranks, the k leading columns gathered into the outputs; info_host filled.  Returns the worst status.
static int direct_finalize(const Direct& c, const Progress& pr, float* const* U_host, float* const* S_host, float* const* V_host, int64_t k,
                           int* info_host) {
    const Plan& p = c.p; const int batch = p.batch; const hipStream_t st = c.st;
    {
        ProfScope ps(4, st);
        if (p.vmode == 2) {
            const int64_t ops = (int64_t)p.m_pad * PB;
            backsolve_kernel<<<dim3((unsigned)ceil_div64(p.nb, 4), (unsigned)ceil_div64(p.nb, 4), batch), 256, 0, st>>>(
                (const float*)(c.wb + p.off_xorig), ops, ops * p.nb, c.X, p.panel_stride, p.batch_stride, p.nb, p.m_pad);
        }
        colnorm_kernel<<<dim3(p.nb, batch), 256, 0, st>>>(c.X, p.panel_stride, p.batch_stride, p.m_pad, p.R, p.n_pad, c.sig, c.ina, c.inv);
        rank_kernel<<<dim3((unsigned)ceil_div64(p.n_pad, 256), batch), 256, 0, st>>>(c.sig, p.n_pad, c.perm);
        for (int b = 0; b < batch; ++b) {
            float* Uo = U_host ? U_host[b] : nullptr;
            float* Vo = V_host ? V_host[b] : nullptr;
            // oriented left vectors (A part) are U of A when not transposed, V of A when transposed
            float* outA = p.transposed ? Vo : Uo;
            float* outV = p.transposed ? Uo : Vo;
            const int rowsA = outA ? p.rows : 0;
            const int rowsV = (p.vmode != 0 && outV) ? p.cols : 0;   // V rows exist only when the right vectors were requested
            dim3 grid((unsigned)ceil_div64(k, 64), (unsigned)ceil_div64(rowsA + rowsV > 0 ? rowsA + rowsV : 1, 64));
            gather_kernel<<<grid, 256, 0, st>>>(c.X + (int64_t)b * p.batch_stride, p.panel_stride, p.m_pad, p.R,
                                                c.sig + (int64_t)b * p.n_pad, c.ina + (int64_t)b * p.n_pad,
                                                c.inv + (int64_t)b * p.n_pad, c.perm + (int64_t)b * p.n_pad, rowsA, rowsV,
                                                (int)k, outA, outV, S_host[b]);
        }
    }
    ASVD_HIP_CHECK(hipStreamSynchronize(st));
    ASVD_HIP_CHECK(hipGetLastError());

    int worst = ASVD_OK;
    for (int b = 0; b < batch; ++b) {
        if (info_host) {
            info_host[4 * b + 0] = pr.status[b];
            info_host[4 * b + 1] = pr.sweeps[b];
            info_host[4 * b + 2] = pr.last_rot[b];
            std::memcpy(&info_host[4 * b + 3], &pr.last_off[b], sizeof(float));  // last sweep's max scaled off-diagonal (float bits)
        }
        if (pr.status[b] > worst) worst = pr.status[b];
    }
    return worst;
}

// One direct call; its arguments are those asvd_svd_batched has checked.  allow_f16: the fused update + Gram kernel of the dense sweeps
// (split-fp16 arithmetic with power-of-two column scales taken from the carried column norms, twolevel.h).  When a problem turned NaN on that
// path nothing is finalised: the call is repeated with the separate passes (fp32 Gram pass, split-bf16 update pass), which need no scales — a
// NaN that is in the data comes back as NaN.
static int svd_direct(int batch, const void* const* a_host, int a_dtype, int64_t m, int64_t n, int64_t lda,
                      const void* const* cs_host, int cs_dtype, float* const* U_host, float* const* S_host,
                      float* const* V_host, int64_t k, int max_sweeps, float tol, void* work, size_t work_bytes,
                      int* info_host, void* stream, bool allow_f16 = true) {
    Direct c;
    // the right vectors of the oriented problem are V of A (not transposed) or U of A (transposed)
    if (int rc = make_plan(batch, m, n, (m < n ? U_host : V_host) != nullptr, c.p)) return rc;
    if (work_bytes < c.p.total) return ASVD_E_WORKSPACE;
    if (max_sweeps <= 0) max_sweeps = 30;
    if (!(tol > 0.0f)) tol = 1e-6f;
    direct_bind(c, work, (hipStream_t)stream, k, tol);
    const Plan& p = c.p;
    if (int rc = direct_pack(c, a_host, a_dtype, lda, cs_host, cs_dtype)) return rc;

    // a two-level dense sweep runs only its internal step d = 1 through the single-level kernels (it also refreshes the carried diagonal
    // blocks); its super-steps follow
    const std::vector<int> steps = p.two ? std::vector<int>{0} : single_level_schedule(c.nsteps);
    std::vector<int> flags((size_t)batch * 4, 0);
    Progress pr(batch);
    SparseLists sl;
    bool sparse = false, fused_used = false;
    for (int sweep = 0; sweep < max_sweeps; ++sweep) {
        const auto t0 = std::chrono::steady_clock::now();
        ASVD_HIP_CHECK(hipMemsetAsync(c.maxoff, 0, (size_t)batch * sizeof(int), c.st));
        ASVD_HIP_CHECK(hipMemsetAsync(c.nrot, 0, (size_t)batch * sizeof(int), c.st));
        ASVD_HIP_CHECK(hipMemsetAsync(c.nupd, 0, (size_t)batch * sizeof(int), c.st));
        long long marked = 0;
        if (sparse) {
            if (int rc = sparse_snapshot(c, pr.done, sl, &marked, t0)) return rc;
            sparse_rounds(c, sl);
        } else {
            single_level_steps(c, steps, p.two);
            if (int rc = p.two ? super_steps(c, allow_f16, &fused_used) : ASVD_OK) return rc;
        }
        ASVD_HIP_CHECK(hipMemcpyAsync(flags.data(), c.wb + p.off_flags, (size_t)batch * 4 * sizeof(int), hipMemcpyDeviceToHost, c.st));
        ASVD_HIP_CHECK(hipStreamSynchronize(c.st));
        note_sweep(p, pr, flags, sweep, sparse, marked, ms_since(t0));
        bool changed = false;
        if (update_convergence(pr, flags, sweep, c.tol, &changed)) break;
        sparse = next_sweep_sparse(p, pr);
        if (changed) {
            ASVD_HIP_CHECK(hipMemcpyAsync(c.done, pr.done.data(), (size_t)batch * sizeof(int), hipMemcpyHostToDevice, c.st));
            ASVD_HIP_CHECK(hipStreamSynchronize(c.st));  // pr.done may be modified next sweep
        }
    }

    for (int b = 0; b < batch && fused_used; ++b)
        if (pr.status[b] == ASVD_N_NAN) {
            debug_trace("problem %d turned NaN on the split-fp16 path: repeating the call with the separate passes", b);
            g_last_path |= ASVD_PATH_PLAIN_RETRY;
            return svd_direct(batch, a_host, a_dtype, m, n, lda, cs_host, cs_dtype, U_host, S_host, V_host, k, max_sweeps, tol, work, work_bytes, info_host,
                              stream, false);
        }
    return direct_finalize(c, pr, U_host, S_host, V_host, k, info_host);
}

static bool nn_i8_wanted() {
    const char* e = getenv("ASVD_NN_I8");   // read per call
    return !(e && atoi(e) == 0);
}
static bool gram_i8_wanted() {
    const char* e = getenv("ASVD_GRAM_I8");   // read per call: tests and A/B runs toggle it inside one process
    return !(e && atoi(e) == 0);
}

// G (upper 32-blocks) = X^T X of the packed panels through the int8 digit planes (gram_i8.h).  scratch: >= 3 * n_pad * 64 * batch bytes; the
// rows go in segments of what fits (and of at most 32768 rows: the int32 accumulators), each added to G in fp64.  ex: n_pad column exponents per
// problem (colmaxexp_kernel) in the order of X.  inv / exs / dp (all or none): column q of X goes to plane position inv[q], exs / dp are the exponents and
// norms in plane order, and G_ij / (dp_i dp_j) is stored — the sorted, unit-scaled Gram matrix the Cholesky factorisation starts from, without a pass
// over an unsorted one.
static int launch_gram_i8(const float* Xp, int64_t panel_stride, int64_t batch_stride, int nb, int m_pad, int n_pad, int batch, double* G,
                          int64_t ldg, int64_t gbs, signed char* scratch, size_t scratch_bytes, const int* ex, const int* inv, const int* exs,
                          const double* dp, int seg_rows_max, hipStream_t st) {
    int64_t cap_rows = (int64_t)(scratch_bytes / ((size_t)3 * n_pad * batch)) / 64 * 64;
    if (cap_rows > 32768) cap_rows = 32768;
    if (seg_rows_max >= 64 && cap_rows > seg_rows_max / 64 * 64) cap_rows = seg_rows_max / 64 * 64;
    if (cap_rows < 64) return ASVD_E_WORKSPACE;
    const int64_t m64 = round_up64(m_pad, 64);
    const int nseg = (int)ceil_div64(m64, cap_rows);
    const int seg = (int)round_up64(ceil_div64(m64, nseg), 64);
    ASVD_HIP_CHECK(hipFuncSetAttribute((const void*)gram_i8_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, GI_LDS_BYTES));
    const int nt = (nb + 3) / 4, ntri = nt * (nt + 1) / 2;
    for (int s = 0; s < nseg; ++s) {
        const int r0 = s * seg;
        const int rows = (int)std::min<int64_t>(seg, m64 - r0);
        if (rows <= 0) break;
        const int kgs = rows / 16;
        const int64_t plane_stride = (int64_t)nb * kgs * 512;
        split_i8_kernel<<<dim3(nb, (unsigned)ceil_div64(kgs, 8), batch), 256, 0, st>>>(Xp, panel_stride, batch_stride, nb, m_pad, n_pad, ex, r0, kgs,
                                                                                       scratch, plane_stride, inv, nullptr);
        gram_i8_kernel<<<dim3(ntri, batch), 512, GI_LDS_BYTES, st>>>(scratch, plane_stride, nb, kgs, n_pad, inv ? exs : ex, G, ldg, gbs, s > 0 ? 1 : 0, nt,
                                                                           dp);
    }
    ASVD_HIP_CHECK(hipGetLastError());
    return ASVD_OK;
}

struct TallLayout {
    size_t off_xp, off_g, off_gs, off_dp, off_df, off_perm, off_dg, off_d, off_fail, off_r, off_vr, off_part, off_inv, off_bex, off_aex, off_vmax, off_gex, off_ex, off_exs, off_cinv, off_inner, inner_bytes, total;
    int n_pad64;
};

static int tall_layout(int batch, const Plan& p, int want_vectors, int64_t k, TallLayout& t) {
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    t.n_pad64 = p.n_pad;  // n_pad is a multiple of 64 = Cholesky block
    t.off_xp = take((size_t)p.m_pad * PB * p.nb * batch * sizeof(float));
    t.off_g = take((size_t)p.n_pad * p.n_pad * batch * sizeof(double));
    t.off_gs = take((size_t)p.n_pad * p.n_pad * batch * sizeof(double));
    t.off_dp = take((size_t)p.n_pad * batch * sizeof(double));
    t.off_df = take((size_t)p.n_pad * batch * sizeof(float));
    t.off_perm = take((size_t)p.n_pad * batch * sizeof(int));
    t.off_dg = take((size_t)(p.n_pad / CB) * CB * CB * batch * sizeof(double));
    t.off_d = take((size_t)p.n_pad * batch * sizeof(double));
    t.off_fail = take((size_t)batch * sizeof(int));
    t.off_r = take((size_t)p.n_pad * p.n_pad * batch * sizeof(float));
    t.off_vr = take(want_vectors ? (size_t)2 * p.cols * k * batch * sizeof(float) : 0);  // permuted + un-permuted right vectors
    t.off_part = take(want_vectors ? (size_t)64 * k * batch * sizeof(double) : 0);  // per problem: the epilogues run on side streams
    t.off_inv = take(want_vectors ? (size_t)k * batch * sizeof(float) : 0);
    // column exponents of the int8 Gram matrix (gram_i8.h), original and sorted order
    t.off_ex = take((size_t)p.n_pad * batch * sizeof(int));
    t.off_exs = take((size_t)p.n_pad * batch * sizeof(int));
    t.off_cinv = take((size_t)p.n_pad * batch * sizeof(int));   // plane position of every column (inverse of the norm sort)
    // exponents of the int8 long-side product (nn_gemm_i8.h): columns of X, rows of X, columns of Vr (key of the maximum, then the exponent)
    t.off_bex = take(want_vectors ? (size_t)p.n_pad * batch * sizeof(int) : 0);
    t.off_aex = take(want_vectors ? (size_t)round_up64(p.m_pad, 128) * batch * sizeof(int) : 0);
    t.off_vmax = take(want_vectors ? (size_t)round_up64(k, 32) * batch * sizeof(unsigned) : 0);
    t.off_gex = take(want_vectors ? (size_t)round_up64(k, 32) * batch * sizeof(int) : 0);
    Plan pi;
    int rc = make_plan(batch, p.cols, p.cols, want_vectors, pi);
    if (rc) return rc;
    t.inner_bytes = pi.total;
    t.off_inner = take(pi.total);
    t.total = off;
    return ASVD_OK;
}

static size_t tall_worksize(int batch, int64_t m, int64_t n, int want_vectors, int64_t k) {
    Plan p;
    if (make_plan(batch, m, n, 0, p)) return 0;
    TallLayout t;
    if (tall_layout(batch, p, want_vectors, k, t)) return 0;
    return t.total;
}


// Y = X Vr for the problems [b0, b0 + zb) of the epilogue on the int8 matrix pipe (nn_gemm_i8.h).  Digit planes: Vr in the G region, X^T (row
// segments of what fits) in the Gs region — both free since R left them; exponents in their own small arrays.
static int launch_nn_i8(const Plan& p, const TallLayout& t, char* wb, const TallBatch& tb, int b0, int zb, int64_t k, hipStream_t st) {
    const float* Xz = (const float*)(wb + t.off_xp) + (int64_t)b0 * p.batch_stride;
    const double* d = (const double*)(wb + t.off_d);
    int* bex = (int*)(wb + t.off_bex) + (int64_t)b0 * p.n_pad;
    const int rows_pad = (int)round_up64(p.m_pad, 128), kp = (int)round_up64(k, 32);
    int* aex = (int*)(wb + t.off_aex) + (int64_t)b0 * rows_pad;
    unsigned* vmax = (unsigned*)(wb + t.off_vmax) + (int64_t)b0 * kp;
    int* gex = (int*)(wb + t.off_gex) + (int64_t)b0 * kp;
    const int cgs = p.n_pad / 16, jps = kp / 32;
    const int64_t strideB = (int64_t)jps * cgs * 512;
    signed char* planesB = (signed char*)(wb + t.off_g);
    signed char* planesA = (signed char*)(wb + t.off_gs);
    colexp_from_norm_kernel<<<(unsigned)ceil_div64((int64_t)p.n_pad * zb, 256), 256, 0, st>>>(d + (int64_t)b0 * p.n_pad, p.n_pad * zb, bex);
    rowmaxexp_kernel<<<dim3((unsigned)(rows_pad / 8), zb), 256, 0, st>>>(Xz, p.panel_stride, p.batch_stride, p.nb, p.rows, rows_pad, bex, p.n_pad, aex);
    ASVD_HIP_CHECK(hipMemsetAsync(vmax, 0, (size_t)kp * zb * sizeof(unsigned), st));
    const int vchunks = (int)std::min<int64_t>(32, ceil_div64(p.cols, 64));
    const int vrpc = (int)ceil_div64(p.cols, vchunks);
    vcolmax_kernel<<<dim3((unsigned)ceil_div64(k, 256), vchunks, zb), 256, 0, st>>>(tb, p.cols, (int)k, k, bex, p.n_pad, vrpc, vmax, kp);
    split_v_i8_kernel<<<dim3(jps, (unsigned)ceil_div64(cgs, 8), zb), 256, 0, st>>>(tb, p.cols, (int)k, k, bex, p.n_pad, vmax, kp, cgs, planesB, strideB, gex);
    ASVD_HIP_CHECK(hipFuncSetAttribute((const void*)nn_gemm_i8_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, GI_LDS_BYTES));
    int64_t seg = ((int64_t)8 * p.n_pad / 3) / 128 * 128;   // rows of X^T planes per problem that fit the Gs region
    if (seg > rows_pad) seg = rows_pad;
    for (int64_t r0 = 0; r0 < rows_pad; r0 += seg) {
        const int rps = (int)(std::min<int64_t>(seg, rows_pad - r0) / 32);
        // seg and rows_pad are multiples of 128, so every block of the segment holds four real row panels: nn_gemm_i8_kernel tests rows only
        // against p.rows, and a clamped A panel (gi_tile_loop) inside a segment would be stored
        if (rps < 4 || (rps & 3)) return ASVD_E_BADARG;
        const int64_t strideA = (int64_t)rps * cgs * 512;
        split_xt_i8_kernel<<<dim3(rps, (unsigned)ceil_div64(cgs, 8), zb), 256, 0, st>>>(Xz, p.panel_stride, p.batch_stride, p.rows, rows_pad, bex, p.n_pad,
                                                                                      aex, (int)r0, cgs, planesA, strideA);
        const int gx = (int)ceil_div64(jps, 4), gy = (int)ceil_div64(rps, 4);
        nn_gemm_i8_kernel<<<dim3(gx * gy, zb), 512, GI_LDS_BYTES, st>>>(tb, planesA, strideA, rps, planesB, strideB, jps, cgs, aex, rows_pad, gex, kp,
                                                                             (int)r0, p.rows, (int)k, k, gx, gy);
    }
    return ASVD_OK;
}

// The reduction of the tall path: pack, G = X^T X, columns sorted by decreasing norm, sorted Cholesky-QR.  Leaves R (fp32) at t.off_r, the
// column order at t.off_perm and the column norms at t.off_d.  NOT_APPLICABLE when the Cholesky breaks down.
static int tall_reduce(const Plan& p, const TallLayout& t, char* wb, const void* const* a_host, int a_dtype, int64_t lda, const void* const* cs_host,
                       int cs_dtype, hipStream_t st) {
    const int batch = p.batch;
    float* Xp = (float*)(wb + t.off_xp);
    double *G = (double*)(wb + t.off_g), *Gs = (double*)(wb + t.off_gs), *d = (double*)(wb + t.off_d), *Dg = (double*)(wb + t.off_dg), *dp = (double*)(wb + t.off_dp);
    float* dF = (float*)(wb + t.off_df);
    int* cperm = (int*)(wb + t.off_perm);
    int* fail = (int*)(wb + t.off_fail);
    float* R = (float*)(wb + t.off_r);
    const int64_t ldg = p.n_pad, gbs = (int64_t)p.n_pad * p.n_pad;
    const int nbk = p.n_pad / CB;
    {
        ProfScope ps(0, st);
        ASVD_HIP_CHECK(hipMemsetAsync(Xp, 0, (size_t)p.batch_stride * batch * sizeof(float), st));
        ASVD_HIP_CHECK(hipMemsetAsync(fail, 0, (size_t)batch * sizeof(int), st));
        if (int prc = pack_batch(a_host, a_dtype, lda, cs_host, cs_dtype, p, Xp, st)) return prc;
    }
    // G = X^T X: exact integer arithmetic on the int8 matrix pipe (gram_i8.h), or the fp64 matrix instructions (ASVD_GRAM_I8=0), then
    // sort columns by decreasing norm (stable, padding last; 14 -> 10 sweeps, unsorted saves nothing), permute + unit-scale the Gram matrix.
    // The int8 path takes the norms from the data first (fp64, colmaxexp_kernel) and stores the sorted, scaled matrix directly: Gs = D^-1 P^T G~ P D^-1
    // with G~ the exact Gram matrix of the digitised columns and D the norms of the original ones — diagonal 1 + O(1e-7) instead of exactly 1,
    // which is a column scaling like any other (R is un-scaled with the same D).  Digit planes in the G region, which this path does not use.
    // A Cholesky breakdown on the int8 path is retried ONCE with the fp64 Gram matrix before the call gives up on the reduction: the digitised columns
    // differ from X by ~2^-25 of their largest entry, which decides the sign of a pivot only where singular values sit at the fp32 rounding level of
    // X itself (rank n/4 + 1e-4 noise under abs_mean scaling: `profiles/r6_families.txt`) — there the exact Gram matrix of the exact X still factors.
    std::vector<int> hfail(batch, 0);
    bool use_i8 = gram_i8_wanted();
    for (int attempt = 0; attempt < 2; ++attempt) {
        {
            ProfScope ps(0, st);
            if (attempt) ASVD_HIP_CHECK(hipMemsetAsync(fail, 0, (size_t)batch * sizeof(int), st));
            if (use_i8) {
                int* ex = (int*)(wb + t.off_ex);
                int* exs = (int*)(wb + t.off_exs);
                colmaxexp_kernel<<<dim3(p.nb, batch), 256, 0, st>>>(Xp, p.panel_stride, p.batch_stride, p.m_pad, p.n_pad, ex, d);
                d_to_float_kernel<<<(unsigned)ceil_div64((int64_t)p.n_pad * batch, 256), 256, 0, st>>>(d, p.n_pad * batch, dF);
                rank_kernel<<<dim3((unsigned)ceil_div64(p.n_pad, 256), batch), 256, 0, st>>>(dF, p.n_pad, cperm);
                int* cinv = (int*)(wb + t.off_cinv);
                perm_gather_kernel<<<dim3((unsigned)ceil_div64(p.n_pad, 256), batch), 256, 0, st>>>(ex, d, cperm, p.n_pad, exs, dp, cinv);
                if (int rc = launch_gram_i8(Xp, p.panel_stride, p.batch_stride, p.nb, p.m_pad, p.n_pad, batch, Gs, ldg, gbs, (signed char*)G,
                                            (size_t)gbs * batch * sizeof(double), ex, cinv, exs, dp, 0, st))
                    return rc;
            } else {
                gram64_kernel<<<dim3(p.nb, (unsigned)ceil_div64(p.nb, 4), batch), 256, 0, st>>>(Xp, p.panel_stride, p.batch_stride, p.nb, p.m_pad, G, ldg, gbs);
                chol_diag_kernel<<<dim3((unsigned)ceil_div64(p.n_pad, 256), batch), 256, 0, st>>>(G, ldg, gbs, p.n_pad, d);
                d_to_float_kernel<<<(unsigned)ceil_div64((int64_t)p.n_pad * batch, 256), 256, 0, st>>>(d, p.n_pad * batch, dF);
                rank_kernel<<<dim3((unsigned)ceil_div64(p.n_pad, 256), batch), 256, 0, st>>>(dF, p.n_pad, cperm);
                g_permute_scale_kernel<<<dim3((unsigned)ceil_div64(p.n_pad, 256), p.n_pad, batch), 256, 0, st>>>(G, ldg, gbs, d, cperm, p.n_pad, Gs, dp);
            }
            // block rows in groups of six (four until round 6): inside a group each finished row updates the rest of the group's strip (K = 64), the matrix
            // behind the group is updated once per group (K = 384)
            // (Round 6, measured and removed — profiles/r6_chol_lookahead.txt: the chain of group g + 1 on a second, equally CU-masked stream beside the bulk
            // of group g's trailing update, the next group's strip updated first.  Reduction 48.1-48.5 -> 52.3 ms per 32 x 4096^2: the two extra launches and
            // event hand-overs per group cost more than the 0.5 ms chain they hide, and the trailing update loses the CUs the chain occupies.)
            // (block rows per group, 32 x 4096^2, reduction ms: 2: 48.0 · 4: 44.4-44.6 · 5: 42.1 · 6: 42.2-42.6 · 7: 41.9 · 8: 44.9-45.2 — profiles/r6_chol_group.txt)
            constexpr int cg = 6;
            for (int j0 = 0; j0 < nbk; j0 += cg) {
                const int j1 = std::min(nbk, j0 + cg);
                for (int jb = j0; jb < j1; ++jb) {
                    chol_diag_wave_kernel<<<batch, 64, 0, st>>>(Gs, ldg, gbs, jb, fail, Dg, nbk);
                    if (jb + 1 < nbk) chol_trsm_kernel<<<dim3(nbk - jb - 1, batch), 256, 0, st>>>(Gs, ldg, gbs, jb);
                    if (jb + 1 < j1) chol_syrk_kernel<<<dim3(j1 - jb - 1, nbk - jb - 1, batch), 256, 0, st>>>(Gs, ldg, gbs, jb, nbk);
                }
                if (j1 < nbk) chol_syrk_multi_kernel<<<dim3(nbk - j1, nbk - j1, batch), 256, 0, st>>>(Gs, ldg, gbs, j0, j1 - j0, nbk);
            }
            r_to_f32_t_kernel<<<dim3((unsigned)(p.n_pad / 32), (unsigned)(p.n_pad / 32), batch), 256, 0, st>>>(Gs, ldg, gbs, Dg, dp, p.n_pad, R, gbs);  // n_pad is a multiple of 64
        }
        ASVD_HIP_CHECK(hipMemcpyAsync(hfail.data(), fail, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, st));
        ASVD_HIP_CHECK(hipStreamSynchronize(st));
        bool broke = false;
        for (int b = 0; b < batch; ++b) broke = broke || hfail[b];
        if (!broke) break;
        if (use_i8 && attempt == 0) {
            debug_trace("Cholesky breakdown on the int8 Gram matrix: once more with the fp64 Gram matrix");
            use_i8 = false;
            g_last_path |= ASVD_PATH_GRAM_RETRY;
            continue;
        }
        break;
    }
    for (int b = 0; b < batch; ++b)
        if (hfail[b]) {
            debug_trace("Cholesky-QR breakdown for problem %d (code %d): falling back to the direct path", b, hfail[b]);
            return NOT_APPLICABLE;
        }
    return ASVD_OK;
}

// The vectors of the tall path: right vectors un-permuted, long-side vectors X v / sigma, sigma refined to |X v|, up to TALL_ZB problems per
// launch.  vperm / vr: right vectors in sorted-column / original order.
static int tall_epilogue(const Plan& p, const TallLayout& t, char* wb, const std::vector<float*>& vperm, const std::vector<float*>& vr,
                         float* const* U_host, float* const* S_host, float* const* V_host, int64_t k, hipStream_t st) {
    const int batch = p.batch;
    const float* Xp = (const float*)(wb + t.off_xp);
    const int* cperm = (const int*)(wb + t.off_perm);
    ProfScope ps(4, st);
    const int nsp = (int)std::min<int64_t>(64, ceil_div64(p.rows, 256));
    const int rps = (int)ceil_div64(p.rows, nsp);
    for (int b0 = 0; b0 < batch; b0 += TALL_ZB) {
        const int zb = std::min(TALL_ZB, batch - b0);
        TallBatch tb{};
        bool any_long = false;
        for (int z = 0; z < zb; ++z) {
            const int b = b0 + z;
            tb.vperm[z] = vperm[b];
            tb.vr[z] = vr[b];
            tb.lng[z] = p.transposed ? (V_host ? V_host[b] : nullptr) : (U_host ? U_host[b] : nullptr);
            tb.S[z] = S_host[b];
            any_long = any_long || tb.lng[z];
        }
        row_unpermute_kernel<<<dim3((unsigned)ceil_div64(k, 256), p.cols, zb), 256, 0, st>>>(tb, cperm + (int64_t)b0 * p.n_pad, p.n_pad, p.cols, (int)k);
        if (!any_long) continue;
        if (nn_i8_wanted() && p.cols <= 32768) {
            if (int rc = launch_nn_i8(p, t, wb, tb, b0, zb, k, st)) return rc;
        } else {
            nn_gemm_split_kernel<<<dim3((unsigned)ceil_div64(k, 128), (unsigned)ceil_div64(p.rows, 128), zb), 256, 0, st>>>(
                tb, Xp + (int64_t)b0 * p.batch_stride, p.panel_stride, p.batch_stride, p.nb, p.rows, p.cols, k, (int)k, k);
        }
        // sigma_j = |X v_j| and unit left vectors
        double* part = (double*)(wb + t.off_part) + (size_t)b0 * 64 * k;
        float* invs = (float*)(wb + t.off_inv) + (size_t)b0 * k;
        colsumsq_kernel<<<dim3((unsigned)ceil_div64(k, 64), nsp, zb), 256, 0, st>>>(tb, k, p.rows, (int)k, rps, part, (int64_t)64 * k);
        colfinish_kernel<<<zb, 256, 0, st>>>(tb, part, (int64_t)64 * k, nsp, (int)k, invs);
        colscale_kernel<<<dim3((unsigned)ceil_div64(k, 256), (unsigned)ceil_div64(p.rows, 32), zb), 256, 0, st>>>(tb, k, p.rows, (int)k, invs);
    }
    ASVD_HIP_CHECK(hipStreamSynchronize(st));
    ASVD_HIP_CHECK(hipGetLastError());
    return ASVD_OK;
}

// The tall path: reduction, Jacobi on R^T (the direct driver), vectors.  NOT_APPLICABLE when the reduction is not (Cholesky breakdown, workspace):
// the caller then runs the direct path.
static int svd_tall(int batch, const void* const* a_host, int a_dtype, int64_t m, int64_t n, int64_t lda, const void* const* cs_host,
                    int cs_dtype, float* const* U_host, float* const* S_host, float* const* V_host, int64_t k, int max_sweeps,
                    float tol, void* work, size_t work_bytes, int* info_host, void* stream) {
    Plan p;
    int rc = make_plan(batch, m, n, 0, p);  // panels hold the A rows only
    if (rc) return rc;
    const int want_vectors = (U_host || V_host) ? 1 : 0;
    TallLayout t;
    rc = tall_layout(batch, p, want_vectors, k, t);
    if (rc) return rc;
    if (work_bytes < t.total) return NOT_APPLICABLE;
    hipStream_t st = (hipStream_t)stream;
    char* wb = (char*)work;
    // Jacobi runs on R^T: the leading right vectors of X are then the directly rotated columns (orthogonal to 1e-6) instead of
    // backsolved ones, which matters because the long-side vectors X v / sigma amplify the error of v by sigma_1 / sigma_j;
    // row-scaled problems (wide layers: the activation scales sit on the long side) also need 3 fewer sweeps.
    rc = tall_reduce(p, t, wb, a_host, a_dtype, lda, cs_host, cs_dtype, st);
    if (rc) return rc;

    // right vectors of X = right vectors of R  (left vectors of R^T): written straight to the caller's short-side output when it exists, else
    // to the temporary
    const int64_t gbs = (int64_t)p.n_pad * p.n_pad;
    float* R = (float*)(wb + t.off_r);
    float* Vr = (float*)(wb + t.off_vr);
    std::vector<const void*> rp(batch);
    std::vector<float*> vr(batch, nullptr), vperm(batch, nullptr);
    for (int b = 0; b < batch; ++b) {
        rp[b] = R + (int64_t)b * gbs;
        if (want_vectors) {
            float* short_out = p.transposed ? (U_host ? U_host[b] : nullptr) : (V_host ? V_host[b] : nullptr);
            vperm[b] = Vr + (int64_t)(2 * b) * p.cols * k;                       // right vectors in sorted-column order
            vr[b] = short_out ? short_out : Vr + (int64_t)(2 * b + 1) * p.cols * k;  // ... in the original order
        }
    }
    float* const* inner_U = want_vectors ? vperm.data() : nullptr;   // left vectors of R^T = right vectors of X
    rc = svd_direct(batch, rp.data(), ASVD_F32, p.cols, p.cols, p.n_pad, nullptr, 0, inner_U, S_host, nullptr, k, max_sweeps, tol,
                    wb + t.off_inner, t.inner_bytes, info_host, stream);
    if (rc < 0) return rc;
    if (want_vectors) {
        if (int erc = tall_epilogue(p, t, wb, vperm, vr, U_host, S_host, V_host, k, st)) return erc;
    }
    return rc;
}

// ---- a batch as two halves on disjoint halves of the chip --------------------------------------------------------------------------------
// The two launches that alternate through a dense sweep use complementary resources — the eigen-solves the VALUs (no HBM), the fused update +
// Gram kernel the HBM path (VALUs nearly idle) — but they cannot share a CU (2 x 216 + 215 VGPRs per SIMD against the 512 of the register
// file), and two half-batches that share the WHOLE chip fall into lock-step (each kernel fills every CU as soon as it is free): 608 vs 628 ms.
// What does overlap them is SPACE: every half gets its own 128 CUs (hipExtStreamCreateWithCUMask) and its own host thread, the halves
// drift apart, and while one is in a compute-bound phase (eigen-solves, fp64 Cholesky-QR, snapshots, the long-side GEMM) the other's
// HBM-bound launches have the memory system to themselves — the fused kernel reaches 72 % of its full-chip throughput on half of the CUs
// (it saturates the HBM path at ~190 CUs: profiles/r5_cu_mask_scaling.jsonl).  Measured, 32 x 4096^2: 628 -> 595 ms (-5.3 %); 11008 x 4096
// and 4096 x 11008 x 32: -5 %; 2048-column problems: nothing (profiles/r5_ab_two_streams.jsonl).  So: batches of >= 4 problems with
// >= 3072 columns are split unless ASVD_SPLIT=0; a profiled call (asvd_svd_set_profiling) runs unsplit, so that the per-class
// durations describe each kernel alone on the chip.  The halves are ordinary calls with disjoint workspaces and outputs (the
// concurrency contract of the library), sized for 128 CUs; results are those of two half-batch calls.
// What the split owns (include/asvd_hip.h, "Ownership"): per CALLING HOST THREAD and device, created at that thread's first split call and
// released when the thread ends — two CU-masked streams and ONE worker thread (the second half runs on it; the first half on the calling
// thread).  Per thread, not per process: two host threads that make split calls at the same time each have their own pair of streams, so their
// calls stay independent and — what tests/test_gpu_concurrency.py holds the library to — whether a call is split never depends on timing.
struct SplitCtx {
    hipStream_t s[2] = {nullptr, nullptr};
    int dev = -1;
    int cus = 0;            // CUs of one half
    bool ok = false;
    std::mutex m;
    std::condition_variable cv;
    std::function<void()> job;
    bool has_job = false, job_done = false, stop = false;
    std::thread worker;
    ~SplitCtx() {
        if (worker.joinable()) {
            { std::lock_guard<std::mutex> lk(m); stop = true; }
            cv.notify_all();
            worker.join();
        }
        for (int h = 0; h < 2; ++h)
            if (s[h]) (void)hipStreamDestroy(s[h]);
    }
};
struct SplitTls { std::vector<std::unique_ptr<SplitCtx>> v; };
static thread_local SplitTls g_split_tls;
static std::mutex g_split_mutex;
static std::atomic<int> g_split_mode{-1};   // asvd_svd_set_split: -1 environment / automatic, 0 never, 1 automatic

static void split_worker(SplitCtx* c) {
    (void)hipSetDevice(c->dev);
    std::unique_lock<std::mutex> lk(c->m);
    for (;;) {
        c->cv.wait(lk, [&] { return c->has_job || c->stop; });
        if (c->stop) return;
        std::function<void()> job = std::move(c->job);
        c->has_job = false;
        lk.unlock();
        try { job(); } catch (...) {}   // the job reports through the variables it captured; nothing may cross the thread boundary
        lk.lock();
        c->job_done = true;
        c->cv.notify_all();
    }
}

static SplitCtx* split_ctx() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    for (auto& c : g_split_tls.v)
        if (c->dev == dev) return c->ok ? c.get() : nullptr;
    g_split_tls.v.emplace_back(new SplitCtx());
    SplitCtx* c = g_split_tls.v.back().get();
    c->dev = dev;
    const int ncu = device_cus();
    if (ncu < 64 || (ncu & 1)) return nullptr;
    const int words = (ncu + 31) / 32;
    bool ok = true;
    for (int h = 0; h < 2 && ok; ++h) {
        std::vector<uint32_t> mask((size_t)words, 0u);
        for (int cu = h * (ncu / 2); cu < (h + 1) * (ncu / 2); ++cu) mask[cu >> 5] |= 1u << (cu & 31);
        ok = hipExtStreamCreateWithCUMask(&c->s[h], (uint32_t)words, mask.data()) == hipSuccess;
    }
    c->cus = ncu / 2;
    if (ok) {
        try { c->worker = std::thread(split_worker, c); } catch (...) { ok = false; }
    }
    c->ok = ok;
    return ok ? c : nullptr;
}

// Presence of this process on a device: one byte of /dev/shm/asvd_hip_split.<pci bus id>, taken as a POSIX record lock at the first
// asvd_svd_batched call on that device (the lock is gone when the process exits, however it exits; the descriptor stays open for the life of the
// process).  F_GETLK reports only locks of OTHER processes: that is how two ranks on one GPU (`--same_gpu`) see each other — both would otherwise
// claim "the first half + the second half" of the CUs and oversubscribe every one of them.
static int g_presence_fd[64];
static std::atomic<int> g_presence_state[64];   // 0 not tried, 1 registered, 2 unavailable (no /dev/shm, no bus id): treated as alone
static void presence_register(int dev) {
    if (dev < 0 || dev >= 64 || g_presence_state[dev].load(std::memory_order_acquire) != 0) return;
    std::lock_guard<std::mutex> lk(g_split_mutex);
    if (g_presence_state[dev].load(std::memory_order_relaxed) != 0) return;
    int state = 2;
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus) - 1, dev) == hipSuccess) {
        for (char* q = bus; *q; ++q) if (*q == ':' || *q == '/') *q = '_';
        char path[128];
        snprintf(path, sizeof(path), "/dev/shm/asvd_hip_split.%s", bus);
        const int fd = open(path, O_CREAT | O_RDWR | O_CLOEXEC, 0666);
        if (fd >= 0) {
            bool mine = false;
            for (int slot = 0; slot < 256 && !mine; ++slot) {
                struct flock fl {};
                fl.l_type = F_WRLCK; fl.l_whence = SEEK_SET; fl.l_start = slot; fl.l_len = 1;
                mine = fcntl(fd, F_SETLK, &fl) == 0;
            }
            if (mine) { g_presence_fd[dev] = fd; state = 1; } else close(fd);
        }
    } else (void)hipGetLastError();
    g_presence_state[dev].store(state, std::memory_order_release);
}
static bool split_device_shared(int dev) {
    if (dev < 0 || dev >= 64 || g_presence_state[dev].load(std::memory_order_acquire) != 1) return false;
    struct flock fl {};
    fl.l_type = F_WRLCK; fl.l_whence = SEEK_SET; fl.l_start = 0; fl.l_len = 256;
    if (fcntl(g_presence_fd[dev], F_GETLK, &fl) != 0) return false;
    return fl.l_type != F_UNLCK;
}

// a caller whose own stream is already restricted to a subset of the CUs has partitioned the chip itself: its calls are not split again
static bool stream_is_cu_masked(hipStream_t st) {
    const int ncu = device_cus();
    uint32_t mask[16] = {0};
    const int words = std::min(16, (ncu + 31) / 32);
    if (hipExtStreamGetCUMask(st, (uint32_t)words, mask) != hipSuccess) { (void)hipGetLastError(); return false; }
    int bits = 0;
    for (int w = 0; w < words; ++w) bits += __builtin_popcount(mask[w]);
    return bits > 0 && bits < ncu;
}

static bool split_applies(int batch, int64_t m, int64_t n) {
    const int mode = g_split_mode.load(std::memory_order_relaxed);
    if (mode == 0) return false;
    if (mode < 0) {
        const char* e = getenv("ASVD_SPLIT");   // read per call: tests and A/B runs toggle it inside one process
        if (e && atoi(e) == 0) return false;
    }
    return batch >= 4 && std::min(m, n) >= 3072;   // measured: 4 x 4096^2 -3 %, 8: -8 %, 12: -6 %, 16: -9 %, 32: -6 %; 2048 columns: nothing
}


static bool reduce_wanted(int64_t m, int64_t n) {
    // The reduction pays for every shape: for tall problems it shrinks each Jacobi step from rows x cols to cols x cols, and for all
    // of them the norm-sorted Cholesky-QR is a preconditioner (Jacobi on R^T: 14 -> 10 sweeps at 4096^2, better orthogonality).
    if (getenv("ASVD_NO_REDUCE")) return false;
    return std::min(m, n) >= 128;
}

// workspace of ONE call of `batch` problems whose launches are sized for the CUs of the current thread (call_cus_now())
static int worksize_one(int batch, int64_t m, int64_t n, int want_vectors, size_t* bytes) {
    Plan p;
    int rc = make_plan(batch, m, n, want_vectors, p);
    if (rc) return rc;
    size_t need = p.total;  // the direct path is always available as the fallback
    if (reduce_wanted(m, n)) {
        const size_t t = tall_worksize(batch, m, n, want_vectors, p.cols);
        if (t > need) need = t;
    }
    *bytes = need;
    return ASVD_OK;
}

// g_call_cus overridden for the life of a scope
struct CallCusScope {
    int saved;
    explicit CallCusScope(int cus) : saved(g_call_cus) { g_call_cus = cus; }
    ~CallCusScope() { g_call_cus = saved; }
};

// workspaces of the two halves of a split batch, each planned for `cus` CUs: half 0 takes h0 bytes from the start, half 1 h1 bytes from off1
static int split_worksizes(int batch, int64_t m, int64_t n, int want_vectors, int cus, size_t* h0, size_t* h1, size_t* off1) {
    CallCusScope cs(cus);
    int rc = worksize_one((batch + 1) / 2, m, n, want_vectors, h0);
    if (!rc) rc = worksize_one(batch / 2, m, n, want_vectors, h1);
    *off1 = (*h0 + 255) & ~(size_t)255;
    return rc;
}

// One call on one stream: the reduced path where it applies, else (or when it breaks down) the direct path.  prof_base: see Profile::end.
static int svd_batched_one(int batch, const void* const* a_host, int a_dtype, int64_t m, int64_t n, int64_t lda,
                           const void* const* cs_host, int cs_dtype, float* const* U_host, float* const* S_host,
                           float* const* V_host, int64_t k, int max_sweeps, float tol, void* work, size_t work_bytes,
                           int* info_host, void* stream, hipEvent_t prof_base) {
    if (g_prof.on) g_prof.begin();
    int rc = NOT_APPLICABLE;
    g_last_path = 0;
    if (reduce_wanted(m, n)) {
        rc = svd_tall(batch, a_host, a_dtype, m, n, lda, cs_host, cs_dtype, U_host, S_host, V_host, k, max_sweeps, tol, work, work_bytes,
                      info_host, stream);
        g_last_path |= (rc == NOT_APPLICABLE) ? ASVD_PATH_REDUCE_FALLBACK : ASVD_PATH_REDUCED;
    }
    if (rc == NOT_APPLICABLE)
        rc = svd_direct(batch, a_host, a_dtype, m, n, lda, cs_host, cs_dtype, U_host, S_host, V_host, k, max_sweeps, tol, work, work_bytes,
                        info_host, stream);
    if (g_prof.on) g_prof.end(prof_base);
    return rc;
}

// The batch as two halves (see SplitCtx): the first (batch + 1) / 2 problems on the calling thread and stream s[0], the rest on the worker
// thread and s[1].  Returns the result of the two calls, SPLIT_REFUSED, or NOT_APPLICABLE (the workspace does not hold both halves).
static int svd_split(int batch, const void* const* a_host, int a_dtype, int64_t m, int64_t n, int64_t lda,
                     const void* const* cs_host, int cs_dtype, float* const* U_host, float* const* S_host,
                     float* const* V_host, int64_t k, int max_sweeps, float tol, void* work, size_t work_bytes,
                     int* info_host, void* stream) {
    SplitCtx* ss = split_ctx();
    if (!ss) return SPLIT_REFUSED;
    const int nb0 = (batch + 1) / 2, nb1 = batch / 2;
    size_t h0 = 0, h1 = 0, off1 = 0;
    if (split_worksizes(batch, m, n, (U_host || V_host) ? 1 : 0, ss->cus, &h0, &h1, &off1) || work_bytes < off1 + h1) return NOT_APPLICABLE;
    // not when another process computes on this device, not on a caller's CU-masked stream: such a call runs as ONE call on the caller's stream
    int dev = 0;
    ASVD_HIP_CHECK(hipGetDevice(&dev));
    if (split_device_shared(dev) || stream_is_cu_masked((hipStream_t)stream)) return SPLIT_REFUSED;

    const bool prof = g_prof.on;
    // everything the caller queued on its stream (weights, scale vectors) is visible to both halves
    hipEvent_t ev;
    ASVD_HIP_CHECK(hipEventCreateWithFlags(&ev, prof ? hipEventDefault : hipEventDisableTiming));
    ASVD_HIP_CHECK(hipEventRecord(ev, (hipStream_t)stream));
    ASVD_HIP_CHECK(hipStreamWaitEvent(ss->s[0], ev, 0));
    ASVD_HIP_CHECK(hipStreamWaitEvent(ss->s[1], ev, 0));
    hipEvent_t base = prof ? ev : nullptr;
    int rc1 = ASVD_E_HIP, path1 = 0;
    Profile prof1;   // the worker's record of half 1
    {
        std::lock_guard<std::mutex> lk(ss->m);
        ss->job = [&]() {
            CallCusScope cs(ss->cus);
            g_prof.on = prof;
            try {
                rc1 = svd_batched_one(nb1, a_host + nb0, a_dtype, m, n, lda, cs_host ? cs_host + nb0 : nullptr, cs_dtype, U_host ? U_host + nb0 : nullptr,
                                      S_host + nb0, V_host ? V_host + nb0 : nullptr, k, max_sweeps, tol, (char*)work + off1, h1,
                                      info_host ? info_host + 4 * nb0 : nullptr, (void*)ss->s[1], base);
            } catch (...) { rc1 = ASVD_E_HIP; }
            path1 = g_last_path;
            prof1 = std::move(g_prof);
            g_prof = Profile{};
        };
        ss->has_job = true;
        ss->job_done = false;
    }
    ss->cv.notify_all();
    int rc0 = ASVD_E_HIP;
    {
        CallCusScope cs(ss->cus);
        try {
            rc0 = svd_batched_one(nb0, a_host, a_dtype, m, n, lda, cs_host, cs_dtype, U_host, S_host, V_host, k, max_sweeps, tol, work, h0, info_host,
                                  (void*)ss->s[0], base);
        } catch (...) { rc0 = ASVD_E_HIP; }
    }
    {
        std::unique_lock<std::mutex> lk(ss->m);
        ss->cv.wait(lk, [&] { return ss->job_done; });
    }
    g_last_path |= path1 | ASVD_PATH_SPLIT;
    (void)hipStreamSynchronize(ss->s[0]);
    (void)hipStreamSynchronize(ss->s[1]);
    if (prof) {   // the halves one by one, their sums as the call's profile
        g_split_prof.last = true;
        for (int h = 0; h < 2; ++h) {
            std::memcpy(g_split_prof.ms[h], (h ? prof1 : g_prof).ms, sizeof(g_prof.ms));
            std::memcpy(g_split_prof.launches[h], (h ? prof1 : g_prof).launches, sizeof(g_prof.launches));
        }
        g_prof.add(prof1);
        class8_overlap(g_prof.iv8, prof1.iv8, g_split_prof.overlap);
    }
    (void)hipEventDestroy(ev);
    if (rc0 < 0) return rc0;
    if (rc1 < 0) return rc1;
    return std::max(rc0, rc1);
}

static int svd_batched_entry(int batch, const void* const* a_host, int a_dtype, int64_t m, int64_t n, int64_t lda,
                             const void* const* cs_host, int cs_dtype, float* const* U_host, float* const* S_host,
                             float* const* V_host, int64_t k, int max_sweeps, float tol, void* work, size_t work_bytes,
                             int* info_host, void* stream) {
    if (!a_host || !S_host || !work || !dtype_ok(a_dtype) || lda < n) return ASVD_E_BADARG;
    if (cs_host && !dtype_ok(cs_dtype)) return ASVD_E_BADARG;
    if (batch < 1 || m < 1 || n < 1 || m > MAX_DIM || n > MAX_DIM) return ASVD_E_BADARG;
    if (k < 1 || k > std::min(m, n)) return ASVD_E_BADARG;
    for (int b = 0; b < batch; ++b)
        if (!a_host[b] || !S_host[b]) return ASVD_E_BADARG;
    {
        int dev0 = 0;
        if (hipGetDevice(&dev0) == hipSuccess) presence_register(dev0);
    }
    // two halves on disjoint halves of the chip (see SplitCtx above)
    g_split_prof.last = false;
    if (split_applies(batch, m, n) && (!g_prof.on || g_prof_keep_split) && g_call_cus == 0) {
        const int rc = svd_split(batch, a_host, a_dtype, m, n, lda, cs_host, cs_dtype, U_host, S_host, V_host, k, max_sweeps, tol, work, work_bytes,
                                 info_host, stream);
        if (rc == SPLIT_REFUSED) {
            const int rcu = svd_batched_one(batch, a_host, a_dtype, m, n, lda, cs_host, cs_dtype, U_host, S_host, V_host, k, max_sweeps, tol, work,
                                            work_bytes, info_host, stream, nullptr);
            g_last_path |= ASVD_PATH_SPLIT_REFUSED;
            return rcu;
        }
        if (rc != NOT_APPLICABLE) return rc;
    }
    return svd_batched_one(batch, a_host, a_dtype, m, n, lda, cs_host, cs_dtype, U_host, S_host, V_host, k, max_sweeps, tol, work, work_bytes, info_host,
                           stream, nullptr);
}

}  // namespace

extern "C" {

void asvd_svd_set_profiling(int enabled) { g_prof.on = enabled != 0; g_prof_keep_split = enabled == 2; }

int asvd_svd_get_profile(float* ms_host, int* launches_host) {
    if (!ms_host || !launches_host) return ASVD_E_BADARG;
    for (int i = 0; i < NPROF; ++i) { ms_host[i] = g_prof.ms[i]; launches_host[i] = g_prof.launches[i]; }
    return ASVD_OK;
}

int asvd_svd_get_split_profile(float* ms_host, int* launches_host, float* overlap_host) {
    if (!ms_host || !launches_host || !overlap_host) return ASVD_E_BADARG;
    for (int h = 0; h < 2; ++h)
        for (int i = 0; i < NPROF; ++i) { ms_host[h * NPROF + i] = g_split_prof.ms[h][i]; launches_host[h * NPROF + i] = g_split_prof.launches[h][i]; }
    for (int i = 0; i < 4; ++i) overlap_host[i] = g_split_prof.overlap[i];
    return g_split_prof.last ? 1 : 0;
}

int asvd_svd_get_sweep_times(float* ms_host, long long* rotated_host, int cap) {
    const int n = (int)g_prof.sweep_ms.size();
    for (int i = 0; i < n && i < cap; ++i) {
        if (ms_host) ms_host[i] = g_prof.sweep_ms[i];
        if (rotated_host) rotated_host[i] = g_prof.sweep_rot[i];
    }
    return n;
}

int asvd_svd_get_pair_counts(long long* counts_host) {
    if (!counts_host) return ASVD_E_BADARG;
    std::memcpy(counts_host, g_prof.pairs, sizeof(g_prof.pairs));
    return ASVD_OK;
}

int asvd_svd_get_last_path(void) { return g_last_path; }

// CUs the calls of THIS host thread may use (0 = the whole device): a caller that runs asvd_svd_batched on a CU-masked stream of its own says so
// here, so that the launch geometry (row splits, chunk counts, launch forms) is sized for those CUs; such calls are never split again.
void asvd_svd_set_call_cus(int cus) { g_call_cus = cus > 0 ? cus : 0; }

void asvd_svd_set_split(int mode) { g_split_mode.store(mode < 0 ? -1 : (mode ? 1 : 0), std::memory_order_relaxed); }

int asvd_svd_worksize(int batch, int64_t m, int64_t n, int want_vectors, size_t* bytes) {
    if (!bytes) return ASVD_E_BADARG;
    size_t need = 0;
    int rc = worksize_one(batch, m, n, want_vectors, &need);
    if (rc) return rc;
    if (split_applies(batch, m, n)) {   // room for the two halves, each planned for half of the CUs
        size_t h0 = 0, h1 = 0, off1 = 0;
        rc = split_worksizes(batch, m, n, want_vectors, std::max(1, device_cus() / 2), &h0, &h1, &off1);
        if (rc) return rc;
        need = std::max(need, off1 + h1);
    }
    *bytes = need;
    return ASVD_OK;
}

int asvd_svd_batched(int batch, const void* const* a_host, int a_dtype, int64_t m, int64_t n, int64_t lda,
                     const void* const* cs_host, int cs_dtype, float* const* U_host, float* const* S_host,
                     float* const* V_host, int64_t k, int max_sweeps, float tol, void* work, size_t work_bytes,
                     int* info_host, void* stream) {
    try {   // the host driver allocates (std::vector): nothing may be thrown across the C boundary
        return svd_batched_entry(batch, a_host, a_dtype, m, n, lda, cs_host, cs_dtype, U_host, S_host, V_host, k, max_sweeps, tol, work, work_bytes, info_host,
                                 stream);
    } catch (...) {
        return ASVD_E_HIP;
    }
}

int asvd_svd(const void* a, int a_dtype, int64_t m, int64_t n, int64_t lda, const void* col_scale, int cs_dtype, float* U,
             float* S, float* V, int64_t k, int max_sweeps, float tol, void* work, size_t work_bytes, int* info_host,
             void* stream) {
    const void* ap[1] = {a};
    const void* cp[1] = {col_scale};
    float* up[1] = {U};
    float* sp[1] = {S};
    float* vp[1] = {V};
    return asvd_svd_batched(1, ap, a_dtype, m, n, lda, col_scale ? cp : nullptr, cs_dtype, (U ? up : nullptr), sp,
                            (V ? vp : nullptr), k, max_sweeps, tol, work, work_bytes, info_host, stream);
}

}  // extern "C"

// ---- test hooks ----------------------------------------------------------------------------------------------------------------------------
extern "C" {

// Test hook (tests/test_gpu_twolevel.py): ONE launch of the two-level update kernel (split-bf16) on caller-built panels, so that the kernel
// can be checked against a plain fp64 product.  X: [batch][nb][R][32] fp32 panels; Qfin: [batch][npairs][128*128]; subact: [batch][npairs][4];
// done, nupd: [batch] ints (all device pointers).
int asvd_test_supdate(float* X, int64_t panel_stride, int64_t batch_stride, int ns, int D, int R, int rows_per_wg, const float* Qfin,
                      const int* subact, const int* done, int* nupd, int nchunks, int npairs, int batch, void* stream) {
    if (!X || !Qfin || !subact || !done || !nupd || ns < 2 || D < 1 || R < 32 || (R % 32) || rows_per_wg < 32 || (rows_per_wg % 32)) return ASVD_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const Sched sc = default_sched();
    supdate_split_kernel<<<dim3(nchunks, npairs, batch), 256, 0, st>>>(sc, X, panel_stride, batch_stride, ns, D, R, rows_per_wg, Qfin, subact, done, nupd);
    ASVD_HIP_CHECK(hipGetLastError());
    return ASVD_OK;
}

// Test hook: the Gram matrix of the reduction alone.  mode 0: gram64_kernel; 1: the int8 digit path (scratch / ex as launch_gram_i8, rows in
// segments of at most seg_rows when >= 64).
int asvd_test_gram(const float* Xp, int64_t panel_stride, int64_t batch_stride, int nb, int m_pad, int batch, int mode, int seg_rows, double* G,
                   void* scratch, size_t scratch_bytes, int* ex, void* stream) {
    if (!Xp || !G || nb < 1 || m_pad < 32 || (m_pad % 32) || batch < 1) return ASVD_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int n_pad = nb * PB;
    if (mode == 0) {
        gram64_kernel<<<dim3(nb, (unsigned)ceil_div64(nb, 4), batch), 256, 0, st>>>(Xp, panel_stride, batch_stride, nb, m_pad, G, n_pad, (int64_t)n_pad * n_pad);
        ASVD_HIP_CHECK(hipGetLastError());
        return ASVD_OK;
    }
    if (!scratch || !ex) return ASVD_E_BADARG;
    colmaxexp_kernel<<<dim3(nb, batch), 256, 0, st>>>(Xp, panel_stride, batch_stride, m_pad, n_pad, ex, nullptr);
    return launch_gram_i8(Xp, panel_stride, batch_stride, nb, m_pad, n_pad, batch, G, n_pad, (int64_t)n_pad * n_pad, (signed char*)scratch, scratch_bytes, ex,
                          nullptr, nullptr, nullptr, seg_rows, st);
}

// Test hook: gi_tile_loop alone (i8_digits.h) over every 128 x 128 block of two caller-built plane sets; out: the raw accumulators
// [nw][32 npA][32 npB] (int32).
int asvd_test_i8_tile(const void* planesA, int64_t strideA, int npA, const void* planesB, int64_t strideB, int npB, int kgs, int nw, int* out,
                      void* stream) {
    if (!planesA || !planesB || !out || npA < 1 || npB < 1 || kgs < 4 || (kgs % 4) || kgs > 2048 || (nw != 4 && nw != 5)) return ASVD_E_BADARG;
    if (strideA < (int64_t)npA * kgs * 512 || strideB < (int64_t)npB * kgs * 512) return ASVD_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)ceil_div64(npB, 4), (unsigned)ceil_div64(npA, 4));
    const signed char* pa = (const signed char*)planesA;
    const signed char* pb = (const signed char*)planesB;
    if (nw == 5) {
        ASVD_HIP_CHECK(hipFuncSetAttribute((const void*)i8_tile_test_kernel<5>, hipFuncAttributeMaxDynamicSharedMemorySize, GI_LDS_BYTES));
        i8_tile_test_kernel<5><<<grid, 512, GI_LDS_BYTES, st>>>(pa, strideA, npA, pb, strideB, npB, kgs, out);
    } else {
        ASVD_HIP_CHECK(hipFuncSetAttribute((const void*)i8_tile_test_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, GI_LDS_BYTES));
        i8_tile_test_kernel<4><<<grid, 512, GI_LDS_BYTES, st>>>(pa, strideA, npA, pb, strideB, npB, kgs, out);
    }
    ASVD_HIP_CHECK(hipGetLastError());
    return ASVD_OK;
}

// Test hook: the super-panel pair schedule itself.  out[step * npairs + k] = (S << 16) | T of slot k of super-step `step`, or -1 for an empty
// slot, for the order the library would pick for `ns` super-panels (1 XOR, 2 grouped; see super_pair).  Returns the number of super-steps
// through *nsteps_out.  tests/test_gpu_twolevel.py checks that every pair appears exactly once and that the pairs of a step are disjoint.
int asvd_test_super_schedule(int ns, int grouped, int* out_dev, int out_capacity, int* nsteps_out, int* npairs_out) {
    if (ns < 2 || ns > 1024 || !out_dev || !nsteps_out || !npairs_out) return ASVD_E_BADARG;
    int pw2 = 2;
    while (pw2 < ns) pw2 <<= 1;
    const int npairs = pw2 / 2;
    const bool grp = grouped && grouped_applies(ns);
    const int nsteps = grp ? grouped_steps(ns, group_bits_for(ns)) : pw2 - 1;
    *nsteps_out = nsteps;
    *npairs_out = npairs;
    if ((int64_t)nsteps * npairs > out_capacity || npairs > 1024) return ASVD_E_WORKSPACE;
    Sched sc = default_sched();
    sc.super_order = grp ? 2 : 1;
    if (grp) set_group_table(sc, ns, group_bits_for(ns));
    super_schedule_kernel<<<nsteps, npairs>>>(sc, ns, nsteps, npairs, out_dev);
    ASVD_HIP_CHECK(hipGetLastError());
    ASVD_HIP_CHECK(hipDeviceSynchronize());
    return ASVD_OK;
}

// Test hook: ONE launch of the fused update + next-step Gram kernel (supgram_kernel) on caller-built panels.  Din: [batch][npairs][128] squared column
// norms of every super-pair of step D in Q order (what the eigen-solve launch leaves in EvdV3::Din).  Gx: [batch][npairs][nchunks][6][1024]
// partial tiles of super-step E, indexed by E's pair slots.  E != D, both in [1, 2 * npairs).
int asvd_test_supgram(float* X, int64_t panel_stride, int64_t batch_stride, int ns, int D, int E, int R, int m_pad, int rows_per_wg,
                      const float* Qfin, const int* subact, const float* Din, float* Gx, const int* done, int* nupd, int nchunks, int npairs, int batch,
                      void* stream) {
    if (!X || !Qfin || !subact || !Din || !Gx || !done || !nupd || ns < 3 || npairs < 2 || D < 1 || E < 1 || D == E || D >= 2 * npairs || E >= 2 * npairs ||
        R < 32 || (R % 32) || (m_pad % 32) || rows_per_wg < 32 || (rows_per_wg % 32))
        return ASVD_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    Sched sc = default_sched();
#ifdef ASVD_SG_TIMING
    if (getenv("ASVD_SG_ABLATE")) sc.meas = atoi(getenv("ASVD_SG_ABLATE"));  // tools/bench_supgram.py --timing --ablate N (measurement build only)
#endif
    ASVD_HIP_CHECK(hipFuncSetAttribute((const void*)supgram_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(SUPGRAM_SMEM_FLOATS * sizeof(float))));
    supgram_kernel<<<dim3(nchunks, (2 * npairs) / 4, batch), 512, SUPGRAM_SMEM_FLOATS * sizeof(float), st>>>(sc, X, panel_stride, batch_stride, ns, D, E, R, m_pad,
                                                                                                           rows_per_wg, Qfin, subact, Din, Gx, done, nupd, npairs);
    ASVD_HIP_CHECK(hipGetLastError());
    return ASVD_OK;
}

#ifdef ASVD_SG_TIMING
int asvd_test_sg_timing(unsigned long long* out_host) {  // [2][10] per-stage shader cycles (index 9: tiles) of the last supgram launch (timing builds only)
    ASVD_HIP_CHECK(hipDeviceSynchronize());
    ASVD_HIP_CHECK(hipMemcpyFromSymbol(out_host, HIP_SYMBOL(g_sg_ts), 2 * 10 * sizeof(unsigned long long)));
    return ASVD_OK;
}
#endif

// Test hook (tests/test_gpu_evd_wave.py): the wave-local 64x64 eigen-solver alone.  G: [batch][64][64] symmetric (device); outputs
// Q [batch][64][64] (unsorted, unscaled), diag / rnk / cs [batch][64], Gout [batch][64][64] (the image the sweeps leave), meas [batch][2].
int asvd_test_evd_wave(const float* G, int batch, int sweeps, float* Q, float* diag, int* rnk, float* cs, float* Gout, float* meas, void* stream) {
    if (!G || !Q || !diag || !rnk || !cs || !Gout || !meas || batch < 1) return ASVD_E_BADARG;   // sweeps < 0: |sweeps| cross-only visits on the ring
    launch_evdw_test(batch, (hipStream_t)stream, G, sweeps, Q, diag, rnk, cs, Gout, meas);
    ASVD_HIP_CHECK(hipGetLastError());
    return ASVD_OK;
}

}  // extern "C"
