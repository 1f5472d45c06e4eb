// Rows of the SPD model's all-pairs distance matrix under the three metrics of its vector-valued distance:
//     out[(i - row_begin) N + j] = metric(v(x_i, x_j)) * scale factor,   v_k = log(1 + a_k), a = the eigenvalues of L^-1 (x_j - x_i) L^-T,
// x_i = L L^T, with the pair computed from its block and lane (no pair list).  A kernel of its own beside spd16_coop_kernel (spd.hip)
// and spd_vvd_coop_fwd_kernel (spd_vvd_kernel.hpp), which stay as they are; same routines (spd_coop.hpp, spd_vvd_ql).
//   n <= 5 / SYMPA_FLAG_GENERIC: spd_all_pairs_generic_kernel (spd_allpairs.hip; one lane per pair, spd_math.hpp spd_pair_metric)
//   n = 6..16: spd_all_pairs_kernel<n> -- a wave owns ONE source row i and 64 consecutive columns; the source is loaded and factored
//             once per wave, the sixteen rounds then run the factored front (spd_coop.hpp reduce_pair_front_factored)
// Grid: x = column tile (64 columns), y = source row of this launch (the host splits more than 65 535 rows into launches).
// Instantiated in spd_allpairs_{lo,hi}.hip; launched from spd_allpairs.hip.
#pragma once

#include "siegel_common.hpp"
#include "spd_vvd_kernel.hpp"

namespace sympa_hip {

struct SpdAllPairsArgs {
    const double* table;      // [num_rows, n, n]
    int64_t num_rows;
    int64_t row_begin;        // first row of out
    int64_t row0;             // source row of blockIdx.y == 0 in this launch
    const double* scale;      // device scalar or nullptr
    double inv_scale_coef;
    double* out;              // [row_count, num_rows]
    int32_t* status;
    int metric;               // sympa::METRIC_RIEM / FONE / FINF
    int symmetric;            // full matrix: tiles left of the diagonal tile are skipped, lanes j < i store nothing, j > i store twice
};

constexpr int SPD_ALL_PAIRS_COOP_MIN_N = 6;        // the crossover of the distance kernels (spd.hip)
constexpr unsigned SPD_ALL_PAIRS_MAX_GRID_Y = 65535u;

void launch_spd_all_pairs_coop_lo(const SpdAllPairsArgs& a, int n, dim3 grid, hipStream_t s);      // n = 6..11
void launch_spd_all_pairs_coop_hi(const SpdAllPairsArgs& a, int n, dim3 grid, hipStream_t s);      // n = 12..16

// The epilogue both kernels share: status bits of the pair, NaN for a pair a non-PD point enters, the exact 0 of the diagonal
// (runner.py:152; also for a point that is not positive definite, and without a status bit), the scale, the store(s).
__device__ __forceinline__ void spd_all_pairs_finish(const SpdAllPairsArgs& a, const int64_t i, const int64_t j, double val, const bool ok,
                                                     const bool conv, int& st) {
    if (!ok) { st |= sympa::ST_NOT_PD; val = __builtin_nan(""); }
    if (!conv) st |= sympa::ST_NO_CONVERGENCE;
    if (!sympa::d_finite(val)) st |= sympa::ST_NONFINITE;      // (a NaN compares false)
    if (i == j) { val = 0.0; st = 0; }
    if (a.scale != nullptr) val *= fmax(a.scale[0] * a.inv_scale_coef, 0.1);
    const bool live = j < a.num_rows && (!a.symmetric || j >= i);
    if (live) {
        __builtin_nontemporal_store(val, a.out + (i - a.row_begin) * a.num_rows + j);
        if (a.symmetric && j > i) __builtin_nontemporal_store(val, a.out + j * a.num_rows + i);      // (row_begin = 0 in this mode)
    } else {
        st = 0;
    }
}

// The chosen reduction of v over the eigenvalues d[0 .. M) of one pair, in index order; `ok` collects a_k > -1 (the second point
// is positive definite).  A NaN v_k gives NaN under every metric (fmax alone would drop it).
template <int M>
__device__ __forceinline__ double spd_all_pairs_reduce(const double (&d)[M], const int metric, bool& ok) {
    double acc = 0.0;
    bool nan = false;
#pragma unroll
    for (int k = 0; k < M; ++k) {
        ok = ok && (d[k] > -1.0);
        const double lg = sympa::d_log1p_signed(d[k]);
        nan = nan || !(lg == lg);
        if (metric == sympa::METRIC_RIEM) acc = sympa::d_fma(lg, lg, acc);
        else if (metric == sympa::METRIC_FONE) acc += fabs(lg);
        else acc = fmax(acc, fabs(lg));
    }
    if (metric == sympa::METRIC_RIEM) acc = sympa::d_sqrt(acc);
    return nan ? __builtin_nan("") : acc;
}

// Sixteen lanes per pair for the solves and the first M - TB Householder steps, one lane per pair for the trailing block, the QL
// and the metric: the structure of spd_vvd_coop_fwd_kernel<M> (spd_vvd_kernel.hpp).  One wave per block; the block owns source row
// i = row0 + blockIdx.y and the columns [64 c, 64 c + 64), c = blockIdx.x; lane 16 g + t owns column 64 c + 4 t + g.
//  - The source is factored ONCE per wave: lane r of every group loads row r of x_i (upper triangle, (min, max)), the symmetric row is
//    parked in the wave's LDS (xs[j * 16 + r]: the sixteen lanes of a group read sixteen consecutive doubles, the four groups the same
//    ones), and ldl_rows leaves the unit factor's row and D^-1/2 in registers -- the four groups run it redundantly in the same
//    instruction stream.  A round then loads its column point only, forms y - x against the parked row and takes the PACKED path of
//    spd16_coop_kernel (reduce_pair_front_factored).  The register budget of a round is that of the vvd forward: factor row, y / m,
//    (d, e2), the trailing block.
//  - The QL is spd_vvd_ql (frozen lanes, deflation at eps^2): a lane's value depends on its own pair alone, whatever shares the wave.
//  - A column past the table (j >= N) clamps its load to the last row and stores nothing; in the symmetric mode lanes j < i compute a
//    value nobody stores.  A wave's 64 results are 64 consecutive doubles of one output row; every lane stores its own.
template <int M>
__global__ __launch_bounds__(64, (spd_coop::trailing_block<M>() <= 10 ? 2 : 1)) void spd_all_pairs_kernel(const SpdAllPairsArgs a) {
    using namespace spd_coop;
    constexpr int TB = trailing_block<M>();
    __shared__ __attribute__((aligned(16))) double tile[GROUPS_PER_WAVE * TBUF];
    __shared__ __attribute__((aligned(16))) double xs[N * M];
    __shared__ __attribute__((aligned(16))) double hand_all[GROUPS_PER_WAVE * (TB >= 3 ? TB * TB : 2) + (TB >= 3 ? TB + (TB & 1) : 0)];
    const int64_t i = a.row0 + (int64_t)blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x;
    if (a.symmetric && c < (i >> 6)) return;                       // block-uniform: the tile lies left of the diagonal tile
    const int lane = threadIdx.x;
    const int g = lane >> 4, r = lane & 15;
    double* const hand = hand_all + g * (TB >= 3 ? TB * TB : 2);
    const int64_t j = c * 64 + 4 * r + g;                          // my column
    const int rowj = (int)(j < a.num_rows ? j : a.num_rows - 1);  // num_rows < 2^31 (checked on the host)
    int st = 0;
    // the source: row r of x_i, parked; then its factor row
    double xf[M], rdl;
    {
        const double* px = a.table + (size_t)i * (unsigned)(M * M);
#pragma unroll
        for (int k = 0; k < M; ++k) {
            const int lo = r < k ? r : k, hi = r < k ? k : r;
            xf[k] = px[(hi < M) ? lo * M + hi : 0];               // a phantom lane (r >= M) reads element 0
        }
        if (g == 0) {
#pragma unroll
            for (int k = 0; k < M; ++k) xs[k * N + r] = xf[k];
        }
    }
    const bool pdx = ldl_rows(xf, rdl);
    wave_lds_fence();
    double d[M], e2[M], blk[packed_len<TB>()];
#pragma unroll
    for (int k = 0; k < M; ++k) { d[k] = 0.0; e2[k] = 0.0; }
#pragma unroll
    for (int k = 0; k < packed_len<TB>(); ++k) blk[k] = 0.0;
    for (int t = 0; t < ROUNDS; ++t) {
        double y[M];
        const int rowy = __builtin_amdgcn_ds_bpermute(4 * (16 * g + t), rowj);     // the column of my group's pair
        const double* py = a.table + (size_t)(unsigned)rowy * (unsigned)(M * M);
#pragma unroll
        for (int k = 0; k < M; ++k) {
            const int lo = r < k ? r : k, hi = r < k ? k : r;
            y[k] = py[(hi < M) ? lo * M + hi : 0];
        }
        if constexpr (TB >= 3) {
            wave_lds_fence();
            if (t > 0 && r == t - 1) take_block<TB>(blk, hand);
        }
#pragma unroll
        for (int k = 0; k < M; ++k) y[k] -= xs[k * N + r];         // A = x_j - x_i, exactly 0 on the diagonal pair
        double m[M];
        reduce_pair_front_factored(xf, y, rdl, m, tile + g * TBUF, r);
        wave_lds_fence();
        reduce_pair_back<M, TB>(m, xf, rdl, r, r == t, 0x0001000100010001ull << t, d, e2, hand,
                                hand_all + GROUPS_PER_WAVE * (TB >= 3 ? TB * TB : 2));
    }
    if constexpr (TB >= 3) {
        wave_lds_fence();
        if (r == ROUNDS - 1) take_block<TB>(blk, hand);
    }
    // one pair per lane from here
    if constexpr (TB >= 3) sympa::tridiag_packed<TB>(blk, d + (M - TB), e2 + (M - TB));
    {   // (the QL from the end of the Householder form, as in spd16_coop_kernel)
        double dr[M], er[M];
#pragma unroll
        for (int k = 0; k < M; ++k) { dr[k] = d[M - 1 - k]; er[k] = (k < M - 1) ? e2[M - 2 - k] : 0.0; }
#pragma unroll
        for (int k = 0; k < M; ++k) { d[k] = dr[k]; e2[k] = er[k]; }
    }
    const bool conv = spd_vvd_ql<M>(d, e2);
    bool ok = pdx;
    const double val = spd_all_pairs_reduce<M>(d, a.metric, ok);
    spd_all_pairs_finish(a, i, j, val, ok, conv, st);
    spd_vvd_report(a.status, st, true, lane);
}

}  // namespace sympa_hip
