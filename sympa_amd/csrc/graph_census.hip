// C-ABI sympa_graph_hop_census_rows / sympa_graph_ball_count_rows / sympa_graph_ball_select_rows: exact integer reductions over a
// block of graph distance rows that is already in HBM (sympa_graph_hop_rows, sympa_graph_weighted_rows).  The device side of the
// reference's --subsample and --scale_triplets (train.py:86-93, utils.py:71-102) for graphs whose triplets cannot be listed.
//
// Every kernel looks at the pairs a triplet list holds and no others: row r stands for node i = row_begin + r and only its
// columns j > i count.  All three read a row in words of 64 consecutive columns, one column per lane, the words aligned to
// multiples of 64 so that a wave's load is one contiguous piece; a __ballot turns the word's predicate into a 64-bit mask and
// a popcount counts it.
//   census   the lanes of a word that hold the same distance are found with one ballot per distinct value (hop distances are
//            massively tied: a word rarely holds more than a handful) and ONE lane adds their number to the bin.  Bins below
//            SYMPA_GRAPH_CENSUS_LDS_BINS live in the workgroup's LDS as 64-bit counters and reach the caller's bins in one
//            64-bit global atomic per non-empty bin when the workgroup ends; larger distances go to the global bin directly.
//   count    one workgroup per row; the popcounts of its waves meet in LDS.
//   select   a wave per run of consecutive requests: words are skipped by their popcount until the one that crosses the rank,
//            and inside it the lane whose column has exactly `rank` ball columns below it answers; the next request of the
//            same row goes on from there.
// Integer sums and integer atomics only: no result depends on the grid, the order of the workgroups or the blocking.
#include "siegel_common.hpp"

namespace {
using namespace sympa_hip;

constexpr int CENSUS_BLOCK = 256;
constexpr int CENSUS_CHUNK = 4096;                // columns of one row a workgroup takes at a time
constexpr int CENSUS_UNROLL = 4;                  // words of 64 columns a wave loads before it counts them
constexpr int COUNT_BLOCK = 256;
constexpr int SELECT_BLOCK = 256;                 // four waves per workgroup
constexpr int SELECT_RUN = 16;                    // consecutive requests one wave answers
constexpr int SELECT_UNROLL = 4;                  // words of 64 columns a wave loads before it counts them
typedef unsigned long long u64;

static_assert(SYMPA_GRAPH_CENSUS_LDS_BINS >= 1 && SYMPA_GRAPH_CENSUS_LDS_BINS <= 512, "LDS bins: 1..512");
static_assert(CENSUS_CHUNK % (CENSUS_UNROLL * CENSUS_BLOCK) == 0 && CENSUS_BLOCK % 64 == 0, "whole waves, whole words");

struct CensusArgs {
    const int32_t* hops;
    int64_t ld, row_begin, rows, N, num_bins, chunks;        // chunks: per row
    u64* bins;
};

__global__ __launch_bounds__(CENSUS_BLOCK) void graph_hop_census_kernel(const CensusArgs a) {
    __shared__ u64 s_bins[SYMPA_GRAPH_CENSUS_LDS_BINS];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    for (int b = tid; b < SYMPA_GRAPH_CENSUS_LDS_BINS; b += CENSUS_BLOCK) s_bins[b] = 0;
    __syncthreads();
    const int64_t items = a.rows * a.chunks;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t r = item / a.chunks;
        const int64_t c0 = (item - r * a.chunks) * CENSUS_CHUNK;
        const int64_t i = a.row_begin + r;
        int64_t c1 = c0 + CENSUS_CHUNK;
        c1 = c1 < a.N ? c1 : a.N;
        if (c1 <= i + 1) continue;                                        // the chunk lies left of the diagonal (block-uniform)
        const int32_t* h = a.hops + r * a.ld;
        for (int64_t j0 = c0; j0 < c1; j0 += CENSUS_UNROLL * CENSUS_BLOCK) {       // wave-uniform trip count: the body ballots
            int bin[CENSUS_UNROLL];
#pragma unroll
            for (int w = 0; w < CENSUS_UNROLL; ++w) {                    // the loads of a trip are in flight together
                const int64_t j = j0 + w * CENSUS_BLOCK + tid;
                bin[w] = -1;
                if (j < c1 && j > i) {
                    const int32_t v = h[j];
                    if (v > 0) bin[w] = (int64_t)v < a.num_bins ? v : 0;  // bin 0 counts what the bins cannot hold
                }
            }
#pragma unroll
            for (int w = 0; w < CENSUS_UNROLL; ++w) {
                u64 todo = __ballot(bin[w] >= 0);
                while (todo) {
                    const int leader = __ffsll((long long)todo) - 1;
                    const int lead_bin = __shfl(bin[w], leader);
                    const u64 same = __ballot(bin[w] == lead_bin);
                    if (lane == leader) {
                        const u64 n = (u64)__popcll(same);
                        if (lead_bin < SYMPA_GRAPH_CENSUS_LDS_BINS) atomicAdd(&s_bins[lead_bin], n);
                        else atomicAdd(&a.bins[lead_bin], n);
                    }
                    todo &= ~same;
                }
            }
        }
    }
    __syncthreads();
    for (int b = tid; b < SYMPA_GRAPH_CENSUS_LDS_BINS && (int64_t)b < a.num_bins; b += CENSUS_BLOCK) {
        const u64 n = s_bins[b];
        if (n) atomicAdd(&a.bins[b], n);
    }
}

// a column of the ball: 0 < value <= radius.  -1 (hop rows) and +inf (weighted rows) mark unreachable nodes and fail it, a NaN
// fails it too; the radius is finite.
template <typename T>
__device__ __forceinline__ bool in_ball(const T v, const double radius) {
    return v > (T)0 && (double)v <= radius;
}

template <typename T>
struct BallArgs {
    const T* rows;
    int64_t ld, row_begin, row_count, N;
    double radius;
    int64_t* upper_count;        // count
    const int64_t* req_row;      // select ...
    const int64_t* req_rank;
    int64_t m;
    int64_t* out_col;
    double* out_dist;
    int32_t* status;
};

template <typename T>
__global__ __launch_bounds__(COUNT_BLOCK) void graph_ball_count_kernel(const BallArgs<T> a) {
    __shared__ int64_t s_cnt[COUNT_BLOCK / 64];
    const int tid = threadIdx.x;
    for (int64_t r = blockIdx.x; r < a.row_count; r += gridDim.x) {
        const int64_t i = a.row_begin + r;
        const T* row = a.rows + r * a.ld;
        int64_t cnt = 0;                                                  // the same in every lane of a wave
        for (int64_t j0 = ((i + 1) & ~(int64_t)63); j0 < a.N; j0 += COUNT_BLOCK) {
            const int64_t j = j0 + tid;
            const bool hit = j < a.N && j > i && in_ball(row[j], a.radius);
            cnt += __popcll(__ballot(hit));
        }
        if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
        __syncthreads();
        if (tid == 0) {
            int64_t total = 0;
            for (int w = 0; w < COUNT_BLOCK / 64; ++w) total += s_cnt[w];
            a.upper_count[r] = total;
        }
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(SELECT_BLOCK) void graph_ball_select_kernel(const BallArgs<T> a) {
    const int lane = threadIdx.x & 63;
    const int64_t k0 = ((int64_t)blockIdx.x * (SELECT_BLOCK / 64) + (threadIdx.x >> 6)) * SELECT_RUN;
    // The wave answers SELECT_RUN consecutive requests and keeps its place in the row between them: a request for the same row
    // with a rank at or beyond the ball columns already passed goes on from the current trip (SELECT_UNROLL words, still in
    // registers) instead of from the diagonal.  Requests sorted by (row, rank) therefore cost one scan of a row per wave; any
    // other order only restarts the scan.  Everything that steers the loops is the same in all lanes of the wave.
    int64_t cur_row = -1, j0 = 0, base = 0;                               // base: ball columns of cur_row left of j0
    bool have = false;                                                    // v / mask / cnt hold the trip at j0
    const T* row = a.rows;
    T v[SELECT_UNROLL];
    u64 mask[SELECT_UNROLL];
    int64_t cnt[SELECT_UNROLL], total = 0;
    for (int q = 0; q < SELECT_RUN; ++q) {
        const int64_t k = k0 + q;
        if (k >= a.m) break;
        const int64_t i = a.req_row[k];
        const int64_t rank = a.req_rank[k];
        bool found = false;
        if (i >= a.row_begin && i < a.row_begin + a.row_count && rank >= 0) {
            if (i != cur_row || rank < base) {
                cur_row = i;
                row = a.rows + (i - a.row_begin) * a.ld;
                j0 = (i + 1) & ~(int64_t)63;
                base = 0;
                have = false;
            }
            while (j0 < a.N) {
                if (!have) {
                    total = 0;
#pragma unroll
                    for (int w = 0; w < SELECT_UNROLL; ++w) {            // the loads of a trip are in flight together
                        const int64_t j = j0 + 64 * w + lane;
                        v[w] = (T)0;
                        if (j < a.N && j > i) v[w] = row[j];
                    }
#pragma unroll
                    for (int w = 0; w < SELECT_UNROLL; ++w) {
                        mask[w] = __ballot(in_ball(v[w], a.radius));
                        cnt[w] = __popcll(mask[w]);
                        total += cnt[w];
                    }
                    have = true;
                }
                int64_t left = rank - base;
                if (left < total) {
                    // the trip that crosses the rank: in its word, the lane with exactly `left` ball columns below it answers
#pragma unroll
                    for (int w = 0; w < SELECT_UNROLL; ++w) {
                        if (left >= 0 && left < cnt[w] && ((mask[w] >> lane) & 1ull) &&
                            (int64_t)__popcll(mask[w] & ((1ull << lane) - 1ull)) == left) {
                            a.out_col[k] = j0 + 64 * w + lane;
                            if (a.out_dist != nullptr) a.out_dist[k] = (double)v[w];
                        }
                        left -= cnt[w];
                    }
                    found = true;
                    break;
                }
                base += total;
                j0 += 64 * SELECT_UNROLL;
                have = false;
            }
        }
        if (!found && lane == 0) {
            a.out_col[k] = -1;
            if (a.out_dist != nullptr) a.out_dist[k] = __builtin_nan("");
            if (a.status != nullptr) { atomicOr(&a.status[0], sympa::ST_BAD_INDEX); atomicAdd(&a.status[1], 1); }
        }
    }
}

int check_block(const char* what, const void* rows, int64_t ld, int64_t row_begin, int64_t row_count, int64_t num_nodes, char* msg,
                size_t len) {
    const char* bad = nullptr;
    if (num_nodes <= 0 || num_nodes > (int64_t)0x7fffffff) bad = "num_nodes outside [1, 2^31-1]";
    else if (row_begin < 0 || row_count < 0 || row_begin + row_count > num_nodes) bad = "row block outside the matrix";
    else if (ld < num_nodes) bad = "leading dimension smaller than num_nodes";
    else if (rows == nullptr) bad = "null rows";
    if (bad == nullptr) return 0;
    std::snprintf(msg, len, "%s: %s", what, bad);
    return SYMPA_ERR_BAD_ARG;
}

bool good_radius(const double radius) { return radius >= 0.0 && radius <= 1.79e308; }        // false for a NaN

template <typename T>
int launch_ball(const bool select, const void* rows, int64_t ld, int64_t row_begin, int64_t row_count, int64_t num_nodes,
                double radius, int64_t* upper_count, const int64_t* req_row, const int64_t* req_rank, int64_t m, int64_t* out_col,
                double* out_dist, int32_t* status, void* stream) {
    BallArgs<T> a;
    std::memset(&a, 0, sizeof(a));
    a.rows = reinterpret_cast<const T*>(rows);
    a.ld = ld;
    a.row_begin = row_begin;
    a.row_count = row_count;
    a.N = num_nodes;
    a.radius = radius;
    a.upper_count = upper_count;
    a.req_row = req_row;
    a.req_rank = req_rank;
    a.m = m;
    a.out_col = out_col;
    a.out_dist = out_dist;
    a.status = status;
    if (select) {
        const int64_t per_block = (SELECT_BLOCK / 64) * SELECT_RUN;
        const unsigned grid = (unsigned)((m + per_block - 1) / per_block);
        hipLaunchKernelGGL(graph_ball_select_kernel<T>, dim3(grid), dim3(SELECT_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), a);
    } else {
        const unsigned grid = (unsigned)(row_count < 65536 ? row_count : 65536);
        hipLaunchKernelGGL(graph_ball_count_kernel<T>, dim3(grid), dim3(COUNT_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), a);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail((int)e, hipGetErrorString(e));
    return 0;
}

}  // namespace

extern "C" {

int sympa_graph_hop_census_rows(const int32_t* hops, int64_t ld, int64_t row_begin, int64_t row_count, int64_t num_nodes,
                                int64_t* bins, int64_t num_bins, void* stream) {
    char msg[128];
    if (check_block("graph census", hops, ld, row_begin, row_count, num_nodes, msg, sizeof(msg))) return fail(SYMPA_ERR_BAD_ARG, msg);
    if (num_bins < 1) return fail(SYMPA_ERR_BAD_ARG, "graph census: num_bins must be at least 1");
    if (bins == nullptr || (reinterpret_cast<uintptr_t>(bins) & 7)) return fail(SYMPA_ERR_BAD_ARG, "graph census: bins null or not 8-byte aligned");
    if (row_count == 0) return 0;
    CensusArgs a;
    std::memset(&a, 0, sizeof(a));
    a.hops = hops;
    a.ld = ld;
    a.row_begin = row_begin;
    a.rows = row_count;
    a.N = num_nodes;
    a.num_bins = num_bins;
    a.chunks = (num_nodes + CENSUS_CHUNK - 1) / CENSUS_CHUNK;
    a.bins = reinterpret_cast<u64*>(bins);
    const int64_t items = a.rows * a.chunks;
    const unsigned grid = (unsigned)(items < 2048 ? items : 2048);
    hipLaunchKernelGGL(graph_hop_census_kernel, dim3(grid), dim3(CENSUS_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail((int)e, hipGetErrorString(e));
    return 0;
}

int sympa_graph_ball_count_rows(const void* rows, int rows_fp64, int64_t ld, int64_t row_begin, int64_t row_count,
                                int64_t num_nodes, double radius, int64_t* upper_count, void* stream) {
    char msg[128];
    if (check_block("graph ball count", rows, ld, row_begin, row_count, num_nodes, msg, sizeof(msg))) return fail(SYMPA_ERR_BAD_ARG, msg);
    if (rows_fp64 != 0 && rows_fp64 != 1) return fail(SYMPA_ERR_BAD_ARG, "graph ball count: rows_fp64 must be 0 or 1");
    if (!good_radius(radius)) return fail(SYMPA_ERR_BAD_ARG, "graph ball count: the radius must be finite and not negative");
    if (upper_count == nullptr) return fail(SYMPA_ERR_BAD_ARG, "graph ball count: null upper_count");
    if (row_count == 0) return 0;
    if (rows_fp64) return launch_ball<double>(false, rows, ld, row_begin, row_count, num_nodes, radius, upper_count, nullptr, nullptr, 0,
                                              nullptr, nullptr, nullptr, stream);
    return launch_ball<int32_t>(false, rows, ld, row_begin, row_count, num_nodes, radius, upper_count, nullptr, nullptr, 0, nullptr,
                                nullptr, nullptr, stream);
}

int sympa_graph_ball_select_rows(const void* rows, int rows_fp64, int64_t ld, int64_t row_begin, int64_t row_count,
                                 int64_t num_nodes, double radius, const int64_t* req_row, const int64_t* req_rank, int64_t m,
                                 int64_t* out_col, double* out_dist, int32_t* status, void* stream) {
    char msg[128];
    if (check_block("graph ball select", rows, ld, row_begin, row_count, num_nodes, msg, sizeof(msg))) return fail(SYMPA_ERR_BAD_ARG, msg);
    if (rows_fp64 != 0 && rows_fp64 != 1) return fail(SYMPA_ERR_BAD_ARG, "graph ball select: rows_fp64 must be 0 or 1");
    if (!good_radius(radius)) return fail(SYMPA_ERR_BAD_ARG, "graph ball select: the radius must be finite and not negative");
    if (m < 0 || m > (int64_t)0x7fffffff) return fail(SYMPA_ERR_BAD_ARG, "graph ball select: m outside [0, 2^31-1]");
    if (req_row == nullptr || req_rank == nullptr || out_col == nullptr) return fail(SYMPA_ERR_BAD_ARG, "graph ball select: null buffer");
    if (row_count == 0 || m == 0) return 0;
    if (rows_fp64) return launch_ball<double>(true, rows, ld, row_begin, row_count, num_nodes, radius, nullptr, req_row, req_rank, m,
                                              out_col, out_dist, status, stream);
    return launch_ball<int32_t>(true, rows, ld, row_begin, row_count, num_nodes, radius, nullptr, req_row, req_rank, m, out_col,
                                out_dist, status, stream);
}

}  // extern "C"
