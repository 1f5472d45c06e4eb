// C-ABI sympa_map_rows / sympa_map_workspace_bytes: per-row average precision of a block of distance rows, the ranking half of
// the reference's mean average precision (MeanAveragePrecisionMetric.calculate_metric, sympa/metrics.py:39-63, over the matrix
// Runner.build_distance_matrix assembles, sympa/runner.py:137-154) WITHOUT sorting the row.
//
// Order of row i: self first, then every other column k by the key (d[k], k) -- ascending distance, ties by column index
// (np.argsort(kind="stable")); -0 counts as +0 and NaN sorts after every number.  With the neighbours nbrs(i) ascending by key
// as t = 1..deg, r_t = t + #{non-neighbour columns with a smaller key} and AP_i = mean_t(t / r_t) (NaN when deg = 0).
// A CSR entry equal to its own row is ignored and is no error.  A row with an entry outside [0, num_rows), with more entries
// than max_degree or with rowptr decreasing across it gets ap = NaN and SYMPA_ST_BAD_INDEX (status[1] counts the bad entries,
// one for a bad row length): never the AP of the entries that remain.
//
// One 256-thread workgroup per row (grid-stride over the block's rows):
//   (1) the row's neighbour keys (d[c], c) are gathered into LDS and bitonic-sorted there (deg is usually 2..10);
//   (2) ONE streaming pass over the row with 16-byte loads, four in flight per lane: a column whose key is above the largest
//       neighbour key (the common case in a good embedding) costs a compare; any other one takes a fixed-trip lower-bound
//       search over the sorted keys and, unless it is a neighbour itself (exact key match), adds one to cnt[p] in an LDS
//       histogram at its search position p;
//   (3) r_t = t + cnt[0] + ... + cnt[t-1]; AP = (1/deg) sum_t t / r_t, summed in t order in fp64 by one lane.
// A row with more than MAP_LDS_CAP CSR entries is left to a second kernel of MAP_WIDE_BLOCKS workgroups that runs the same
// steps over a global workspace slice per workgroup (keys, columns, int32 counts): correct for any degree, not fast.
#include "siegel_common.hpp"

namespace {
using namespace sympa_hip;

constexpr int MAP_BLOCK = 256;
// 1 024 entries x (8-byte key + 4-byte column + 4-byte count) = 16 KiB of LDS per workgroup: eight 256-thread workgroups
// (32 waves, the CU's wave limit) take 128 of the 160 KiB, so the cap never limits occupancy.
constexpr int MAP_LDS_CAP = SYMPA_MAP_LDS_CAP;
constexpr int MAP_WIDE_BLOCKS = 16;
constexpr int MAP_UNROLL = 4;            // 16-byte loads in flight per lane in the streaming pass

typedef double v2d_t __attribute__((ext_vector_type(2)));

// order-preserving image of a distance: -0 -> +0, every NaN -> the top; fp32 keys round the value to fp32 first
// (the reference's float32 matrix, runner.py:144)
__device__ __forceinline__ unsigned long long order_key(double d, const bool fp32) {
    if (fp32) d = (double)(float)d;
    if (d != d) return ~0ull;
    if (d == 0.0) d = 0.0;
    const unsigned long long b = (unsigned long long)__double_as_longlong(d);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ bool key_less(unsigned long long ua, int ca, unsigned long long ub, int cb) {
    return ua < ub || (ua == ub && ca < cb);
}

struct MapArgs {
    const double* dist;              // [rows, ld]
    int64_t rows, ld, row_begin, num_rows;
    const int64_t* rowptr;           // [num_rows + 1]
    const int32_t* cols;
    double* ap;                      // [rows]
    int32_t* status;
    int fp32;
    int64_t max_degree;              // the caller's bound on a row's CSR entries (<= the capacity of either kernel)
    int64_t wide_cap;                // entries per workgroup slice of the workspace (wide kernel)
    void* workspace;
};

// keys / cols / cnt: LDS arrays (MAP_LDS_CAP) or one workgroup's workspace slice (wide kernel; counts read back with atomic loads)
template <bool WIDE>
__device__ __forceinline__ void rank_row(const MapArgs& a, const int64_t r, unsigned long long* keys, int* kcol, int* cnt,
                                         int* s_misc) {
    const int tid = threadIdx.x;
    const int64_t g = a.row_begin + r;
    const double* row = a.dist + r * a.ld;
    const int64_t beg = a.rowptr[g], end = a.rowptr[g + 1];
    const int64_t raw = end - beg;
    // the wide kernel's row (block-uniform), unless no wide kernel runs: then the CSR disagrees with max_degree
    if (WIDE ? (raw <= MAP_LDS_CAP) : (raw > MAP_LDS_CAP && a.wide_cap > 0)) return;
    // max_degree <= MAP_LDS_CAP without a wide kernel, <= wide_cap with one: a row within it fits its arrays
    if (raw < 0 || raw > a.max_degree) {                                    // CSR inconsistent with max_degree
        if (tid == 0) {
            a.ap[r] = __builtin_nan("");
            if (a.status != nullptr) { atomicOr(&a.status[0], sympa::ST_BAD_INDEX); atomicAdd(&a.status[1], 1); }
        }
        return;
    }
    int P = 1;
    while (P < raw) P <<= 1;
    if (tid == 0) { s_misc[0] = 0; s_misc[1] = 0; }
    __syncthreads();
    // (1) gather the neighbour keys; self entries become padding (top key), which sorts behind every real key
    int excluded = 0, bad = 0;
    for (int t = tid; t < P; t += MAP_BLOCK) {
        unsigned long long u = ~0ull;
        int c = 0x7fffffff;
        if (t < raw) {
            const int cc = a.cols[beg + t];
            if (cc < 0 || (int64_t)cc >= a.num_rows) { ++bad; ++excluded; }
            else if ((int64_t)cc == g) ++excluded;
            else { u = order_key(row[cc], a.fp32); c = cc; }
        }
        keys[t] = u;
        kcol[t] = c;
        cnt[t] = 0;
    }
    if (excluded) atomicAdd(&s_misc[0], excluded);
    if (bad) {
        atomicAdd(&s_misc[1], bad);
        if (a.status != nullptr) { atomicOr(&a.status[0], sympa::ST_BAD_INDEX); atomicAdd(&a.status[1], bad); }
    }
    __syncthreads();
    if (s_misc[1] != 0) {                                                  // an out-of-range entry: no AP from the rest of the list
        if (tid == 0) a.ap[r] = __builtin_nan("");
        __syncthreads();
        return;
    }
    const int deg = (int)raw - s_misc[0];
    // bitonic sort of the P (key, column) pairs, ascending
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += MAP_BLOCK) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long ui = keys[i], uj = keys[ixj];
                    const int ci = kcol[i], cj = kcol[ixj];
                    const bool up = (i & k) == 0;
                    if (up ? key_less(uj, cj, ui, ci) : key_less(ui, ci, uj, cj)) {
                        keys[i] = uj; keys[ixj] = ui;
                        kcol[i] = cj; kcol[ixj] = ci;
                    }
                }
            }
            __syncthreads();
        }
    }
    if (deg <= 0) {
        if (tid == 0) a.ap[r] = __builtin_nan("");                         // np.mean([]) (metrics.py:61)
        __syncthreads();
        return;
    }
    const unsigned long long mu = keys[deg - 1];
    const int mc = kcol[deg - 1];
    // (2) the streaming pass
    auto visit = [&](const int64_t k, const double d) {
        if (k == g) return;
        const unsigned long long u = order_key(d, a.fp32);
        const int c = (int)k;
        if (u > mu || (u == mu && c > mc)) return;
        int p = 0;
        for (int step = P >> 1; step > 0; step >>= 1)
            if (key_less(keys[p + step - 1], kcol[p + step - 1], u, c)) p += step;
        if (keys[p] == u && kcol[p] == c) return;                           // the neighbour itself
        atomicAdd(&cnt[p], 1);
    };
    const int64_t N = a.num_rows;
    const int64_t head = (reinterpret_cast<uintptr_t>(row) & 15) ? 1 : 0;
    if (head && tid == 0) visit(0, row[0]);
    const int64_t nv = (N - head) >> 1;
    const v2d_t* rv = reinterpret_cast<const v2d_t*>(row + head);
    for (int64_t v0 = tid; v0 < nv; v0 += (int64_t)MAP_BLOCK * MAP_UNROLL) {
        v2d_t x[MAP_UNROLL];
#pragma unroll
        for (int q = 0; q < MAP_UNROLL; ++q) {
            const int64_t v = v0 + (int64_t)q * MAP_BLOCK;
            if (v < nv) x[q] = rv[v];
        }
#pragma unroll
        for (int q = 0; q < MAP_UNROLL; ++q) {
            const int64_t v = v0 + (int64_t)q * MAP_BLOCK;
            if (v < nv) {
                visit(head + 2 * v, x[q].x);
                visit(head + 2 * v + 1, x[q].y);
            }
        }
    }
    if (((N - head) & 1) && tid == 0) visit(N - 1, row[N - 1]);
    __syncthreads();
    // (3) ranks and the mean precision, in t order
    if (tid == 0) {
        int64_t pre = 0;
        double acc = 0.0;
        for (int t = 1; t <= deg; ++t) {
            pre += WIDE ? __hip_atomic_load(&cnt[t - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : cnt[t - 1];
            acc += (double)t / (double)(t + pre);
        }
        a.ap[r] = acc / (double)deg;
    }
    __syncthreads();
}

__global__ __launch_bounds__(MAP_BLOCK) void map_rank_kernel(const MapArgs a) {
    __shared__ unsigned long long keys[MAP_LDS_CAP];
    __shared__ int kcol[MAP_LDS_CAP];
    __shared__ int cnt[MAP_LDS_CAP];
    __shared__ int misc[2];
    for (int64_t r = blockIdx.x; r < a.rows; r += gridDim.x) rank_row<false>(a, r, keys, kcol, cnt, misc);
}

__global__ __launch_bounds__(MAP_BLOCK) void map_rank_wide_kernel(const MapArgs a) {
    __shared__ int misc[2];
    char* base = reinterpret_cast<char*>(a.workspace) + (int64_t)blockIdx.x * a.wide_cap * 16;
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(base);
    int* kcol = reinterpret_cast<int*>(base + a.wide_cap * 8);
    int* cnt = reinterpret_cast<int*>(base + a.wide_cap * 12);
    for (int64_t r = blockIdx.x; r < a.rows; r += gridDim.x) rank_row<true>(a, r, keys, kcol, cnt, misc);
}

int64_t wide_cap_of(int64_t max_degree) {
    int64_t P = 1;
    while (P < max_degree) P <<= 1;
    return P;
}

}  // namespace

extern "C" {

int64_t sympa_map_workspace_bytes(int64_t num_rows, int64_t max_degree) {
    if (num_rows <= 0 || max_degree <= MAP_LDS_CAP) return 0;
    return (int64_t)MAP_WIDE_BLOCKS * wide_cap_of(max_degree) * 16;
}

int sympa_map_rows(const double* dist, int64_t row_count, int64_t ld, int64_t row_begin, int64_t num_rows,
                   const int64_t* rowptr, const int32_t* cols, int64_t max_degree, double* ap, void* workspace,
                   int64_t workspace_bytes, int32_t* status, int flags, void* stream) {
    if (num_rows <= 0 || num_rows > (int64_t)0x7fffffff) return fail(SYMPA_ERR_BAD_ARG, "map: num_rows outside [1, 2^31-1]");
    if (row_begin < 0 || row_count < 0 || row_begin + row_count > num_rows) return fail(SYMPA_ERR_BAD_ARG, "map: row block outside the matrix");
    if (ld < num_rows) return fail(SYMPA_ERR_BAD_ARG, "map: leading dimension smaller than the row length");
    if (max_degree < 0 || max_degree > num_rows) return fail(SYMPA_ERR_BAD_ARG, "map: max_degree outside [0, num_rows]");
    if (flags & ~SYMPA_FLAG_FP32_KEYS) return fail(SYMPA_ERR_BAD_ARG, "map: unknown flags");
    if (row_count == 0) return 0;
    if (dist == nullptr || rowptr == nullptr || ap == nullptr || (cols == nullptr && max_degree > 0))
        return fail(SYMPA_ERR_BAD_ARG, "map: null buffer");
    if (reinterpret_cast<uintptr_t>(dist) & 7) return fail(SYMPA_ERR_BAD_ARG, "map: distance rows not 8-byte aligned");
    const int64_t need = sympa_map_workspace_bytes(num_rows, max_degree);
    if (need > 0 && (workspace == nullptr || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15)))
        return fail(SYMPA_ERR_BAD_ARG, "map: workspace missing, too small or not 16-byte aligned");
    MapArgs a;
    std::memset(&a, 0, sizeof(a));
    a.dist = dist;
    a.rows = row_count;
    a.ld = ld;
    a.row_begin = row_begin;
    a.num_rows = num_rows;
    a.rowptr = rowptr;
    a.cols = cols;
    a.ap = ap;
    a.status = status;
    a.fp32 = (flags & SYMPA_FLAG_FP32_KEYS) ? 1 : 0;
    a.max_degree = max_degree;
    a.wide_cap = need > 0 ? wide_cap_of(max_degree) : 0;
    a.workspace = workspace;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const unsigned grid = (unsigned)(row_count < 65536 ? row_count : 65536);
    hipLaunchKernelGGL(map_rank_kernel, dim3(grid), dim3(MAP_BLOCK), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail((int)e, hipGetErrorString(e));
    if (need > 0) {
        const unsigned wgrid = (unsigned)(row_count < MAP_WIDE_BLOCKS ? row_count : MAP_WIDE_BLOCKS);
        hipLaunchKernelGGL(map_rank_wide_kernel, dim3(wgrid), dim3(MAP_BLOCK), 0, s, a);
        e = hipGetLastError();
        if (e != hipSuccess) return fail((int)e, hipGetErrorString(e));
    }
    return 0;
}

}  // extern "C"
