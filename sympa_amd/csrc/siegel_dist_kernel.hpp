// Kernel templates of the one-pair-per-lane forward (dims 1..8) and their launchers, shared by two translation units:
// siegel_dist.hip instantiates dims 1..4, siegel_dist_big.hip dims 5..8 -- the latter is compiled without the pre-RA machine
// scheduler (-mllvm -enable-misched=0, __graft_entry__.py): the fully unrolled dims-8 kernel then keeps the source order and
// needs 400 fewer v_mov_b64 / 170 fewer v_accvgpr_read (profiles/r03_n8_forward_ab.txt), while the dims <= 4 kernels and the
// fused multi-batch kernel of the headline measured 0-6 % slower without it.
#pragma once
#include "siegel_common.hpp"
#include <hip/hip_ext.h>

namespace sympa_hip {

// Body of one 256-thread block: pairs [first, first + 256) of the batch described by `a`.
// dims 5..8: the bounded model gathers only the chunks that hold upper-triangle elements through three ring buffers, the
// upper model whole rows through two (siegel_gather.hpp: measured per model)
template <int MODEL>
constexpr bool pass_masked() { return MODEL != sympa::MODEL_UPPER; }

template <int N, int MODEL, bool LOWLDS>
struct BlockLds {
    static constexpr bool PASS4 = (N == 4) && LOWLDS;   // minimum-LDS gather: three blocks of different launches per CU
    static constexpr int WAVE_SLOTS = PASS4 ? PASS4_WAVE_SLOTS
                                      : DmaTile<N>::ENABLED ? (LOWLDS ? DmaTile<N>::WAVE_SLOTS_LOW : DmaTile<N>::WAVE_SLOTS)
                                      : (PassTile<N>::ENABLED ? PassTile<N, pass_masked<MODEL>()>::WAVE_SLOTS : Tile<N>::WAVE_SLOTS);
};

// -DSYMPA_HEAD_TIMELINE (a profile build of the dims <= 4 unit, tools/head_timeline.py; never the product build): lane 0 of wave 0
// of every block of the fused multi-batch kernel leaves four shader-clock stamps -- 0 block start, 1 both indices arrived,
// 2 gather complete, 3 in front of the output store -- with the 100 MHz counter at both ends and the place it ran on, eight words
// per block, in the buffer C-ABI sympa_head_timeline_buffer names.  Without the switch HeadTimeline is empty and compiles to nothing.
#ifdef SYMPA_HEAD_TIMELINE
__device__ unsigned long long* g_head_timeline = nullptr;
__device__ unsigned g_head_timeline_blocks = 0;
struct HeadTimeline {
    unsigned long long t[4], r[2];
    template <int K>
    __device__ __forceinline__ void stamp() {   // everything issued so far has arrived, then the clock
        unsigned long long v;
        // (no instruction crosses a stamp: left alone the scheduler moves a third of the arithmetic in front of "gather complete".
        // The profile build therefore runs a few per cent slower than the product, whose schedule is free)
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) :: "memory");
        __builtin_amdgcn_sched_barrier(0);
        t[K] = v;
        if constexpr (K == 0 || K == 3) {
            asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) :: "memory");
            r[K ? 1 : 0] = v;
        }
    }
    __device__ __forceinline__ void store() const {
        unsigned xcc, hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        if (threadIdx.x == 0 && g_head_timeline != nullptr && blockIdx.x < g_head_timeline_blocks) {
            unsigned long long* o = g_head_timeline + 8ull * blockIdx.x;
            o[0] = t[0]; o[1] = t[1]; o[2] = t[2]; o[3] = t[3]; o[4] = r[0]; o[5] = r[1];
            o[6] = (unsigned long long)(xcc & 0xfu) | ((unsigned long long)hw << 8);
            o[7] = 1ull;
        }
    }
};
#else
struct HeadTimeline {
    template <int K>
    __device__ __forceinline__ void stamp() {}
    __device__ __forceinline__ void store() const {}
};
#endif

// Dims 7 and 8 keep the head they had (a search over the prefix ends, one index load behind the other): their kernels sit at the
// 512-register limit, where the new head moved the spills about -- three instantiations gained 36-80 B of scratch, others lost as
// much -- and their waves are alone on a SIMD, with a persistent kernel for the large calls (siegel_packed_kernel.hpp).
constexpr bool new_head(int n) { return n <= 6; }

// The two row indices of this lane's pair, block `first / blockDim.x` of an index list.  The head of every wave waits for these
// loads with nothing to overlap them, so BOTH leave before either is waited for or tested (they are inside the caller's list
// whatever the other one holds), and the address is the block's base -- wave-uniform, scalar registers -- plus a 32-bit lane
// offset instead of a 64-bit multiply per lane and endpoint.  The [b, 2] list form (idx2 == idx1 + 1, stride 2) takes both with
// one 16-byte load.  Index batches stream through once: non-temporal, so they do not evict table rows from L2.
__device__ __forceinline__ void load_index_pair(const DistArgs& a, const int64_t first, int64_t& r1, int64_t& r2) {
    typedef long long v2ll __attribute__((ext_vector_type(2)));
    // pair inside the block; the idle tail lanes repeat the batch's last pair (i < b ? i : b - 1), and no block is empty
    const int64_t rem = a.b - 1 - first;
    const unsigned last = rem < 255 ? (unsigned)rem : 255u;
    const unsigned t = threadIdx.x < last ? threadIdx.x : last;
    const uint64_t s1 = (uint64_t)a.idx1_stride, s2 = (uint64_t)a.idx2_stride;
    if (s1 == 2 && s2 == 2 && a.idx2 == a.idx1 + 1 && (reinterpret_cast<uintptr_t>(a.idx1) & 15) == 0) {
        const char* p = reinterpret_cast<const char*>(a.idx1 + first * 2) + t * 16u;
        const v2ll v = __builtin_nontemporal_load(reinterpret_cast<const v2ll*>(p));
        r1 = v.x;
        r2 = v.y;
    } else if ((s1 | s2) < (1u << 20)) {        // the lane offset fits 32 bits: t * stride * 8 < 2^31
        const char* p1 = reinterpret_cast<const char*>(a.idx1 + first * (int64_t)s1) + t * (unsigned)s1 * 8u;
        const char* p2 = reinterpret_cast<const char*>(a.idx2 + first * (int64_t)s2) + t * (unsigned)s2 * 8u;
        r1 = __builtin_nontemporal_load(reinterpret_cast<const int64_t*>(p1));
        r2 = __builtin_nontemporal_load(reinterpret_cast<const int64_t*>(p2));
    } else {                                    // any other stride of the C-ABI: 64-bit arithmetic per lane
        const int64_t ii = first + t;
        r1 = __builtin_nontemporal_load(a.idx1 + ii * a.idx1_stride);
        r2 = __builtin_nontemporal_load(a.idx2 + ii * a.idx2_stride);
    }
}

// Wave priority of the head of a block of the fused multi-batch kernel, dims 2..4 (0: none; A/B builds: -DSYMPA_HEAD_PRIO=0).
// Four blocks share a CU and the SIMD issues by priority, then AGE: the youngest wave -- the one in its head, whose few address
// instructions gate every gather step -- gets only the slots the three older waves leave.  Raised from block start to "gather
// complete" the head stops waiting behind their arithmetic; it issues almost nothing, so it takes almost nothing from them.
// Measured on the headline on top of the shorter head: -0.11 us per step (profiles/fused_head_ab.txt); 1, 2 and 3 measure the same.
#ifndef SYMPA_HEAD_PRIO
#define SYMPA_HEAD_PRIO 1
#endif

template <int N, int MODEL, bool LOWLDS, bool HEAD_PRIO = false>
__device__ __forceinline__ void dist_block(const DistArgs& a, const int64_t first, v2d* __restrict__ lds, HeadTimeline& tl) {
    constexpr bool PASS4 = BlockLds<N, MODEL, LOWLDS>::PASS4;
    constexpr int WAVE_SLOTS = BlockLds<N, MODEL, LOWLDS>::WAVE_SLOTS;
    // Everything the head reads from the kernel arguments is wanted in registers HERE, in one scalar round trip.  Left alone, each
    // of these loads sits behind the branch that first needs it -- mode, then the list's address, then strides and row count, and the
    // table addresses behind the wait for the indices: four dependent round trips in front of the first gather instruction.
    if constexpr (new_head(N))
        asm volatile("" ::"s"(a.ap_cols), "s"(a.idx1), "s"(a.idx2), "s"(a.idx1_stride), "s"(a.idx2_stride), "s"(a.num_rows), "s"(a.b),
                     "s"(a.base1), "s"(a.base2));
    const int64_t i = first + threadIdx.x;
    const bool live = i < a.b;
    const int64_t ii = live ? i : a.b - 1;   // idle tail lanes recompute the last pair (wave ballots need them)

    int st = 0;
    int64_t r1 = ii, r2 = ii;
    if (a.ap_cols > 0) {          // all-pairs block of the distance matrix (runner.py:142-154)
        ap_pair(a, ii, r1, r2);
    } else if (a.idx1 != nullptr) {
        bool bad;
        if constexpr (new_head(N)) {
            load_index_pair(a, first, r1, r2);
            // one test behind both loads (unsigned: a negative index is a huge one); `|`, not `||`: no branch between the two compares
            bad = ((uint64_t)r1 >= (uint64_t)a.num_rows) | ((uint64_t)r2 >= (uint64_t)a.num_rows);
        } else {
            r1 = __builtin_nontemporal_load(a.idx1 + ii * a.idx1_stride);
            r2 = __builtin_nontemporal_load(a.idx2 + ii * a.idx2_stride);
            bad = r1 < 0 || r1 >= a.num_rows || r2 < 0 || r2 >= a.num_rows;
        }
        if (bad) {
            st |= sympa::ST_BAD_INDEX;
            r1 = 0;
            r2 = 0;
        }
    }
    tl.template stamp<1>();
    constexpr int64_t ROW = 2 * N * N;
    double* vv = (a.vvd != nullptr && live) ? a.vvd + i * N : nullptr;
    double d;
    if constexpr (PassTile<N>::ENABLED) {
        sympa::CMat<N> z1, z2;
        v2d* tile = lds + (threadIdx.x >> 6) * WAVE_SLOTS;
        gather_pair_passes<N, pass_masked<MODEL>()>(a.base1, (int)r1, a.base2, (int)r2, tile, z1, z2);
        d = sympa::pair_distance_mats<N, MODEL>(z1, z2, a.metric, a.metric_w, a.inv_eps, vv, st);
    } else if constexpr (Tile<N>::STAGED) {
        sympa::CMat<N> z1, z2;
        v2d* tile = lds + (threadIdx.x >> 6) * WAVE_SLOTS;
        if constexpr (PASS4)
            gather_pair_pass4(a.base1, (int)r1, a.base2, (int)r2, tile, z1, z2);
        else if constexpr (DmaTile<N>::ENABLED && LOWLDS)
            gather_pair_dma_low<N>(a.base1, (int)r1, a.base2, (int)r2, tile, z1, z2);
        else if constexpr (DmaTile<N>::ENABLED)
            gather_pair_dma_split<N>(a.base1, (int)r1, a.base2, (int)r2, tile, z1, z2);
        else
            gather_pair_staged<N>(a.base1, (int)r1, a.base2, (int)r2, tile, z1, z2);
        if constexpr (HEAD_PRIO) __builtin_amdgcn_s_setprio(0);
        tl.template stamp<2>();
        d = sympa::pair_distance_mats<N, MODEL>(z1, z2, a.metric, a.metric_w, a.inv_eps, vv, st);
    } else {
        d = sympa::pair_distance<N, MODEL>(a.base1 + r1 * ROW, a.base2 + r2 * ROW, a.metric, a.metric_w,
                                           a.inv_eps, vv, st);
    }
    if (st & sympa::ST_BAD_INDEX) d = __builtin_nan("");
    if (a.scale != nullptr) d *= fmax(a.scale[0] * a.inv_scale_coef, 0.1);   // model.py:40-41
    tl.template stamp<3>();
    if (live) {
        if (a.ap_cols > 0) ap_store(a, i, r1, r2, d);
        else __builtin_nontemporal_store(d, a.out + i);
    }

    if (a.status != nullptr) {
        const int flagged = (live && st != 0) ? 1 : 0;
        const unsigned long long m = __ballot(flagged);
        if (m != 0ull) {   // rare path
            if (flagged) atomicOr(&a.status[0], st);
            if ((threadIdx.x & 63) == 0) atomicAdd(&a.status[1], (int)__popcll(m));
        }
    }
}

// Waves per SIMD the compiler must make room for: 1 = one 512-register wave (dims 5, 7, 8).  dims 6, upper: 286 registers by
// itself; held to 256 (two waves per SIMD, 35 registers in scratch) it measures 88.4 -> 83.7 us per 262 144 pairs on the 46.6 MB
// table and 84.4 -> 74.4 us on an L2-resident one (profiles/r03_n6_two_waves.txt).  bounded would spill 163 registers, dims 7 and 8
// several hundred.
template <int N, int MODEL> constexpr int fwd_min_blocks() { return (N == 6 && MODEL == sympa::MODEL_UPPER) ? 2 : 1; }

template <int N, int MODEL, bool LOWLDS>
__global__ __launch_bounds__(fwd_block(N), (fwd_min_blocks<N, MODEL>())) void siegel_dist_kernel(const DistArgs a) {
    __shared__ v2d lds[(fwd_block(N) / 64) * BlockLds<N, MODEL, LOWLDS>::WAVE_SLOTS];
    // Staggered first round (dims 7, 8 on tables that do not fit the L2s; the launcher sets the bit): a lone launch starts one wave
    // on every SIMD at the same instant, all of them gather their 128 KB of rows at once, compute in step and come back for the
    // next round together -- 134 MB bursts on a fabric that then idles.  CU j of every XCD (blocks 32 j .. 32 j + 31 of the first
    // 1 024) starts j x 0.6 us late; the rounds stay out of step from there on.  Upper n = 8, 262 144 pairs, 45 500 rows:
    // 151.1 -> 134.4 us (profiles/r04_fwd_stagger.txt); flat 133.5-134 us for every table from 16 MB up, equal at 10 MB,
    // +4-8 % on L2-resident tables (hence the size test), no gain for the bounded model (more arithmetic per byte).
    if constexpr (N >= 7) {
        if ((a.flags & SYMPA_INTERNAL_FLAG_STAGGER) && blockIdx.x < 1024u) {
            const int k = (int)((blockIdx.x >> 5) & 31u);
            for (int j = 0; j < k; ++j) __builtin_amdgcn_s_sleep(20);
        }
    }
    HeadTimeline tl;
    dist_block<N, MODEL, LOWLDS>(a, (int64_t)blockIdx.x * fwd_block(N), lds, tl);
}

// Several batches in ONE launch (C-ABI sympa_model_forward_batches with SYMPA_FLAG_FUSE): block x belongs to the
// batch k with blk_end[k-1] <= x < blk_end[k]; the batches share table, metric and scale and differ in their index
// list, size and output.  The grid is several blocks per CU deep, so the minimum-LDS gather form is used: three
// blocks of different batches share a CU and one batch's gather hides behind another's arithmetic -- what
// overlapping the launches on streams achieves, without kernel boundaries, fork/join dependencies or idle SIMDs
// when a batch is smaller than one wave per SIMD.
struct MultiArgs {
    DistArgs c;                                    // idx1/idx2/out/b are taken from the lists below
    const int64_t* trip[SYMPA_MAX_FUSED_BATCHES];
    double* out[SYMPA_MAX_FUSED_BATCHES];
    int64_t b[SYMPA_MAX_FUSED_BATCHES];
    unsigned blk_end[SYMPA_MAX_FUSED_BATCHES];     // exclusive prefix end, in blocks; the entries past num_batches hold the grid size
    unsigned uniform_blocks;                       // != 0: every batch has this many blocks, batch of block x = x / uniform_blocks ...
    unsigned uniform_recip;                        // ... = umulhi(x, uniform_recip): multi_uniform_blocks() below
    int num_batches;
};

// uniform_blocks / uniform_recip of a launch whose batches all have `d` blocks (0, 0: the kernel reads the prefix ends).
// m = floor(2^32 / d) + 1 gives floor(x m / 2^32) = floor(x / d) for every x with x d < 2^32; x < 32 d, so d <= 8192 is safe.
// d = 1 has no 32-bit m and is left to the prefix ends.
inline void multi_uniform_blocks(MultiArgs& m, const uint64_t d) {
    m.uniform_blocks = m.uniform_recip = 0u;
    if (d < 2 || d > 8192) return;
    m.uniform_blocks = (unsigned)d;
    m.uniform_recip = (unsigned)(((uint64_t)1 << 32) / d) + 1u;
}

// Waves per SIMD the compiler must make room for in the fused multi-batch kernel (the bounded n = 4 instantiation keeps its 146
// registers = three waves per SIMD: capped at 128 for four it spills 66 and runs 5.39 -> 8.03 us/step, profiles/r03_rejected_variants.txt)
template <int N, int MODEL>
constexpr int multi_min_blocks() { return (N == 6 && MODEL == sympa::MODEL_UPPER) ? 2 : 1; }

template <int N, int MODEL>
__global__ __launch_bounds__(fwd_block(N), (multi_min_blocks<N, MODEL>())) void siegel_dist_multi_kernel(const MultiArgs m) {
    constexpr bool LOW = DmaTile<N>::ENABLED;
    __shared__ v2d lds[(fwd_block(N) / 64) * BlockLds<N, MODEL, LOW>::WAVE_SLOTS];
    constexpr bool HEAD_PRIO = Tile<N>::STAGED && SYMPA_HEAD_PRIO > 0;
    if constexpr (HEAD_PRIO) __builtin_amdgcn_s_setprio(SYMPA_HEAD_PRIO);
    HeadTimeline tl;
    tl.template stamp<0>();
    // Batch of this block (block-uniform, scalar).  The wave can do nothing before it knows its batch, so no chain of dependent
    // loads: equal block counts (the usual list: equal batches) need none at all, k = x / uniform_blocks by the launcher's
    // reciprocal; any other list reads all the prefix ends at once and counts those at or below x in registers (they do not
    // decrease, and the unused ones hold the grid size).  blk_end[k - 1] then travels with trip[k], out[k] and b[k].
    unsigned k, blk0;
    const unsigned ub = m.uniform_blocks, ur = m.uniform_recip;
    // (both wanted in registers here, in one round trip: not the second one behind the branch on the first)
    if constexpr (new_head(N)) asm volatile("" ::"s"(ub), "s"(ur));
    if constexpr (!new_head(N)) {          // (see new_head)
        int lo = 0, hi = m.num_batches - 1;
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            const int mid = (lo + hi) >> 1;
            const bool right = blockIdx.x >= m.blk_end[mid];
            lo = right ? mid + 1 : lo;
            hi = right ? hi : mid;
        }
        k = (unsigned)lo;
        blk0 = (lo == 0) ? 0u : m.blk_end[lo - 1];
    } else if (ub != 0u) {
        k = __umulhi(blockIdx.x, ur);
        blk0 = k * ub;
    } else {
        k = 0u;
#pragma unroll
        for (int i = 0; i < SYMPA_MAX_FUSED_BATCHES - 1; ++i) k += (blockIdx.x >= m.blk_end[i]) ? 1u : 0u;
        blk0 = m.blk_end[k == 0u ? 0u : k - 1u];
        blk0 = (k == 0u) ? 0u : blk0;
    }
    DistArgs a = m.c;
    a.idx1 = m.trip[k];
    a.idx2 = m.trip[k] + 1;
    a.out = m.out[k];
    a.b = m.b[k];
    dist_block<N, MODEL, LOW, HEAD_PRIO>(a, (int64_t)(blockIdx.x - blk0) * fwd_block(N), lds, tl);
    tl.store();
}

// One launch.  SYMPA_FLAG_ANY_ORDER: the dispatch packet carries no barrier bit (hipExtAnyOrderLaunch), so the command
// processor may start it while earlier launches of the SAME stream are still running -- independent steps overlap
// without any cross-stream dependency.
template <typename K>
hipError_t launch_kernel(K kern, unsigned grid, int block, const DistArgs& a, hipStream_t s) {
    if (a.flags & SYMPA_FLAG_ANY_ORDER) {
        void* args[] = {const_cast<DistArgs*>(&a)};
        return hipExtLaunchKernel(reinterpret_cast<const void*>(kern), dim3(grid), dim3(block), args, 0, s, nullptr,
                                  nullptr, hipExtAnyOrderLaunch);
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, s, a);
    return hipGetLastError();
}

// DUAL: the compact-dual instantiations live in units of their own (siegel_dist_dual.hip, siegel_dist_big_dual.hip), so the
// units of the first two models compile exactly the kernels they did before the third existed
template <int N, bool DUAL = false>
int launch_n(const DistArgs& a, int model, hipStream_t s) {
    constexpr int FB = fwd_block(N);
    const unsigned grid = (unsigned)((a.b + FB - 1) / FB);
    DistArgs st = a;
    st.flags &= ~SYMPA_INTERNAL_FLAG_STAGGER;             // an internal bit: never taken from the caller
    if (N >= 7 && model == SYMPA_MODEL_UPPER && a.idx1 != nullptr && a.ap_cols == 0 && grid >= 2048u &&
        a.num_rows * (int64_t)(16 * N * N) >= ((int64_t)12 << 20) && !(a.flags & SYMPA_FLAG_ANY_ORDER))
        st.flags |= SYMPA_INTERNAL_FLAG_STAGGER;          // two rounds or more of a table beyond the L2s: see the kernel
    // low-LDS gather when asked for, or when the grid is deep enough for a second block per CU to matter
    const bool low = DmaTile<N>::ENABLED && ((a.flags & SYMPA_FLAG_LOW_LDS) || grid > 2 * 256 * (BLOCK / FB));
    hipError_t e;
    if constexpr (DUAL) {
        if (low) e = launch_kernel(siegel_dist_kernel<N, sympa::MODEL_DUAL, true>, grid, FB, st, s);
        else e = launch_kernel(siegel_dist_kernel<N, sympa::MODEL_DUAL, false>, grid, FB, st, s);
    } else if (model == SYMPA_MODEL_UPPER) {
        if (low) e = launch_kernel(siegel_dist_kernel<N, sympa::MODEL_UPPER, true>, grid, FB, st, s);
        else e = launch_kernel(siegel_dist_kernel<N, sympa::MODEL_UPPER, false>, grid, FB, st, s);
    } else {
        if (low) e = launch_kernel(siegel_dist_kernel<N, sympa::MODEL_BOUNDED, true>, grid, FB, st, s);
        else e = launch_kernel(siegel_dist_kernel<N, sympa::MODEL_BOUNDED, false>, grid, FB, st, s);
    }
    if (e != hipSuccess) return fail((int)e, hipGetErrorString(e));
    return 0;
}

template <int N, bool DUAL = false>
int launch_multi_n(const MultiArgs& m, unsigned grid, int model, hipStream_t s) {
    if constexpr (DUAL)
        hipLaunchKernelGGL((siegel_dist_multi_kernel<N, sympa::MODEL_DUAL>), dim3(grid), dim3(fwd_block(N)), 0, s, m);
    else if (model == SYMPA_MODEL_UPPER)
        hipLaunchKernelGGL((siegel_dist_multi_kernel<N, sympa::MODEL_UPPER>), dim3(grid), dim3(fwd_block(N)), 0, s, m);
    else
        hipLaunchKernelGGL((siegel_dist_multi_kernel<N, sympa::MODEL_BOUNDED>), dim3(grid), dim3(fwd_block(N)), 0, s, m);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail((int)e, hipGetErrorString(e));
    return 0;
}


// siegel_dist_big.hip: dims 5..8
int launch_dist_big(const DistArgs& a, int n, int model, hipStream_t s);
int launch_multi_big(const MultiArgs& m, unsigned grid, int n, int model, hipStream_t s);
// compact dual, dims 1..8: siegel_dist_dual.hip (1..4), siegel_dist_big_dual.hip (5..8)
int launch_dist_dual(const DistArgs& a, int n, hipStream_t s);
int launch_multi_dual(const MultiArgs& m, unsigned grid, int n, hipStream_t s);
int launch_dist_big_dual(const DistArgs& a, int n, hipStream_t s);
int launch_multi_big_dual(const MultiArgs& m, unsigned grid, int n, hipStream_t s);

}  // namespace sympa_hip
