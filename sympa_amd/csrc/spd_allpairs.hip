// The SPD model's all-pairs distance rows: C-ABI sympa_spd_all_pairs_dist, the dispatch, and the
// one-pair-per-lane kernel (runtime n <= 16, per-lane scratch: n <= 5, and SYMPA_FLAG_GENERIC at every n).  The
// sixteen-lanes-per-pair kernel (spd_allpairs_kernel.hpp) is instantiated in spd_allpairs_{lo,hi}.hip.
#include "spd_allpairs_kernel.hpp"

namespace sympa_hip {
namespace {

// One lane per pair over sympa::spd_pair_metric, the same grid as spd_all_pairs_kernel: block (c, row) owns source row
// i = row0 + row and the columns [64 c, 64 c + 64), lane l column 64 c + l.  The 64 lanes read the same source point (one address
// per instruction); nothing of a lane's arithmetic depends on another lane (tridiag_ql_runtime: a lane that is through does nothing
// more), so a value depends on its own pair alone here as well.
__global__ __launch_bounds__(64) void spd_all_pairs_generic_kernel(const SpdAllPairsArgs a, const int n) {
    const int64_t i = a.row0 + (int64_t)blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x;
    if (a.symmetric && c < (i >> 6)) return;
    const int64_t j = c * 64 + threadIdx.x;
    const int64_t jj = j < a.num_rows ? j : a.num_rows - 1;       // a column past the table: a valid row, nothing stored
    const int nn = n * n;
    int st = 0;
    sympa::SpdWork w;
    const double val = sympa::spd_pair_metric(w, a.table + i * nn, a.table + jj * nn, n, a.metric, st);
    const bool ok = !(st & sympa::ST_NOT_PD), conv = !(st & sympa::ST_NO_CONVERGENCE);
    st = 0;                                                        // (rebuilt from the final value, like the other kernel)
    spd_all_pairs_finish(a, i, j, val, ok, conv, st);
    spd_vvd_report(a.status, st, true, threadIdx.x);
}

}  // namespace
}  // namespace sympa_hip

extern "C" {

int sympa_spd_all_pairs_dist(const double* table, int64_t num_rows, int n, int64_t row_begin, int64_t row_count, int metric,
                             const double* scale, double scale_coef, double* out, int32_t* status, int flags, void* stream) {
    using namespace sympa_hip;
    if (num_rows < 0 || row_begin < 0 || row_count < 0 || row_begin > num_rows || row_count > num_rows - row_begin)
        return fail(SYMPA_ERR_BAD_ARG, "spd all-pairs: row block outside the table");
    if (metric != SYMPA_METRIC_RIEM && metric != SYMPA_METRIC_FONE && metric != SYMPA_METRIC_FINF)
        return fail(SYMPA_ERR_BAD_ARG, "spd all-pairs: metric is SYMPA_METRIC_RIEM, _FONE or _FINF");
    if ((flags & ~(SYMPA_FLAG_GENERIC | SYMPA_FLAG_NO_SYMMETRY)) != 0)
        return fail(SYMPA_ERR_BAD_ARG, "spd all-pairs: flags is 0, SYMPA_FLAG_GENERIC and / or SYMPA_FLAG_NO_SYMMETRY");
    if (n < 1 || n > sympa::SPD_MAX_N) return fail(SYMPA_ERR_UNSUPPORTED_DIMS, "spd: dims outside [1, 16]");
    if (scale != nullptr && !(scale_coef != 0.0)) return fail(SYMPA_ERR_BAD_ARG, "scale_coef must be non-zero");
    if (row_count == 0) return 0;
    if (table == nullptr || out == nullptr) return fail(SYMPA_ERR_BAD_ARG, "null buffer");
    if (num_rows > (int64_t)0x7fffffff) return fail(SYMPA_ERR_BAD_ARG, "more than 2^31-1 table rows");
    SpdAllPairsArgs a;
    std::memset(&a, 0, sizeof(a));
    a.table = table;
    a.num_rows = num_rows;
    a.row_begin = row_begin;
    a.scale = scale;
    a.inv_scale_coef = 1.0 / scale_coef;
    a.out = out;
    a.status = status;
    a.metric = metric;
    a.symmetric = (row_begin == 0 && row_count == num_rows && !(flags & SYMPA_FLAG_NO_SYMMETRY)) ? 1 : 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const unsigned tiles = (unsigned)((num_rows + 63) / 64);
    const bool generic = n < SPD_ALL_PAIRS_COOP_MIN_N || (flags & SYMPA_FLAG_GENERIC);
    for (int64_t done = 0; done < row_count; done += SPD_ALL_PAIRS_MAX_GRID_Y) {
        const int64_t left = row_count - done;
        const dim3 grid(tiles, (unsigned)(left < (int64_t)SPD_ALL_PAIRS_MAX_GRID_Y ? left : (int64_t)SPD_ALL_PAIRS_MAX_GRID_Y));
        a.row0 = row_begin + done;
        if (generic) hipLaunchKernelGGL(spd_all_pairs_generic_kernel, grid, dim3(64), 0, s, a, n);
        else if (n <= 11) launch_spd_all_pairs_coop_lo(a, n, grid, s);
        else launch_spd_all_pairs_coop_hi(a, n, grid, s);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail((int)e, hipGetErrorString(e));
    }
    return 0;
}

}  // extern "C"
