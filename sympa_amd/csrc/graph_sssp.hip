// C-ABI sympa_graph_weighted_rows / sympa_graph_weighted_workspace_bytes / sympa_graph_weighted_distortion_rows: weighted
// shortest-path distances from a block of source nodes to every node of a symmetric CSR graph with non-negative fp64 weights,
// and the distortion of a block of manifold distance rows against them.  The device counterpart of the weighted APSP the
// reference runs in preprocess.py:108-114; the weighted twin of graph_bfs.hip.
//
// out[s][v] is D[s][v] = the minimum over the paths from s to v of the left-to-right fp64 sum of the weights, starting at s.
// fp64 addition of a non-negative weight is monotone and never decreases its left operand, so D[s][.] is what Dijkstra from s
// computes AND the least fixed point of d[v] = min(d[v], min_u fl(d[u] + w(u, v))) from d[s] = 0, +inf elsewhere; every
// relaxation order reaches that fixed point with the same bits.  Rows are NOT symmetric in their last bits (the sum runs from
// the row's own source), so nothing here symmetrises them.
//
// Pull-based multi-source Bellman-Ford.  One workgroup owns a group of K consecutive sources for the whole search and keeps
// one plane [N][K] fp64 (K fastest) in the caller's workspace; a lane owns (node v, source k), so the K lanes of a node read
// the same CSR entries and a neighbour gather is K contiguous doubles.  Relaxation is in place (Gauss-Seidel) through relaxed
// workgroup-scope atomic loads and stores: a stale read inside a sweep only delays convergence.  Sweeps are separated by
// workgroup barriers only; the loop ends when a complete sweep that started after a barrier changed nothing (the block-wide OR
// is that barrier), and its header bounds the trip count by N.  No inter-workgroup synchronisation, no cooperative launch, no
// host round trip per sweep, no atomic read-modify-write on the search path (the status word of a malformed CSR is the one
// exception).  A final pass writes the plane transposed, so every element of the block is written exactly once, in its
// final state.  K = 8; no other value has been timed.
#include "siegel_common.hpp"

namespace {
using namespace sympa_hip;

constexpr int SSSP_BLOCK = 1024;
constexpr int WDST_BLOCK = 256;
constexpr int K = 8;             // sources per workgroup

struct SsspArgs {
    const int64_t* rowptr;
    const int32_t* cols;
    const double* weights;
    int64_t N, E, src_begin, src_count, row_stride;
    double* out;
    double* ws;          // planes: group g at ws + g K N
    int64_t* sweeps;     // [src_count]: the sweeps the group of source r ran
    int32_t* status;
};

__device__ __forceinline__ double relaxed_load(const double* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ void relaxed_store(double* p, const double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ bool weight_ok(const double w) { return w >= 0.0 && w < __builtin_inf(); }      // -0.0 is 0; NaN fails

__global__ __launch_bounds__(SSSP_BLOCK) void graph_sssp_kernel(const SsspArgs a) {
    const int tid = threadIdx.x;
    const int64_t N = a.N;
    const int64_t group = blockIdx.x;
    const int64_t first = a.src_begin + group * K;                       // source of column 0
    const int64_t left = a.src_count - group * K;
    const int nk = left < K ? (int)left : K;
    const int64_t items = N * K;
    double* plane = a.ws + group * K * N;
    const double inf = __builtin_inf();

    // workgroup 0 counts the malformed CSR entries once (the search itself only skips them)
    if (blockIdx.x == 0 && a.status != nullptr) {
        int bad_index = 0, bad_weight = 0;
        for (int64_t v = tid; v < N; v += SSSP_BLOCK) {
            const int64_t beg = a.rowptr[v], end = a.rowptr[v + 1];
            if (beg < 0 || end < beg || end > a.E) ++bad_index;
        }
        for (int64_t e = tid; e < a.E; e += SSSP_BLOCK) {
            const int32_t c = a.cols[e];
            if (c < 0 || (int64_t)c >= N) ++bad_index;
            if (!weight_ok(a.weights[e])) ++bad_weight;
        }
        if (bad_index) atomicOr(&a.status[0], sympa::ST_BAD_INDEX);
        if (bad_weight) atomicOr(&a.status[0], sympa::ST_NONFINITE);
        if (bad_index + bad_weight) atomicAdd(&a.status[1], bad_index + bad_weight);
    }

    // columns past the block's last source stay +inf throughout: their lanes never store
    for (int64_t idx = tid; idx < items; idx += SSSP_BLOCK) {
        const int64_t v = idx / K;
        const int k = (int)(idx % K);
        plane[idx] = (k < nk && v == first + k) ? 0.0 : inf;
    }
    __syncthreads();

    int64_t sweeps = 0;
    for (int64_t sweep = 0; sweep < N; ++sweep) {
        int changed = 0;
        for (int64_t idx = tid; idx < items; idx += SSSP_BLOCK) {
            const int64_t v = idx / K;
            const int k = (int)(idx % K);
            int64_t beg = a.rowptr[v], end = a.rowptr[v + 1];
            beg = beg < 0 ? 0 : beg;
            end = end > a.E ? a.E : end;
            const double old = relaxed_load(plane + idx);
            double best = old;
            for (int64_t e = beg; e < end; ++e) {
                const int32_t c = a.cols[e];
                const double w = a.weights[e];
                if (c >= 0 && (int64_t)c < N && weight_ok(w)) {
                    const double cand = relaxed_load(plane + (int64_t)c * K + k) + w;
                    best = cand < best ? cand : best;
                }
            }
            if (best < old) {
                relaxed_store(plane + idx, best);
                changed = 1;
            }
        }
        ++sweeps;
        if (!__syncthreads_or(changed)) break;
    }

    // the plane is read once, in order; for a fixed k the 8 nodes of a wave store to adjacent addresses of row k
    double* out = a.out + group * K * a.row_stride;
    for (int64_t idx = tid; idx < items; idx += SSSP_BLOCK) {
        const int64_t v = idx / K;
        const int k = (int)(idx % K);
        if (k < nk) out[k * a.row_stride + v] = plane[idx];
    }
    if (tid < nk) a.sweeps[group * K + tid] = sweeps;
}

struct WeightedDistortionArgs {
    const double* dist;      // [rows, ld_dist]
    const double* gdist;     // [rows, ld_g]
    int64_t rows, ld_dist, ld_g, row_begin, N;
    double* sum;             // [rows]
    int64_t* count;          // [rows]
};

// graph_distortion_kernel of graph_bfs.hip over fp64 graph distances: row r (node i = row_begin + r) sums |d - g| / g over the
// columns j > i with 0 < g < inf and counts them.  Lane t adds its columns i + 1 + t, i + 1 + t + 256, ... in order and the 256
// partial sums meet in a fixed tree: the value of a row depends on the row alone.
__global__ __launch_bounds__(WDST_BLOCK) void graph_weighted_distortion_kernel(const WeightedDistortionArgs a) {
    __shared__ double s_sum[WDST_BLOCK];
    __shared__ int64_t s_cnt[WDST_BLOCK];
    const int tid = threadIdx.x;
    for (int64_t r = blockIdx.x; r < a.rows; r += gridDim.x) {
        const int64_t i = a.row_begin + r;
        const double* d = a.dist + r * a.ld_dist;
        const double* g = a.gdist + r * a.ld_g;
        double acc = 0.0;
        int64_t cnt = 0;
        for (int64_t j = i + 1 + tid; j < a.N; j += WDST_BLOCK) {
            const double gd = g[j];
            if (gd > 0.0 && gd < __builtin_inf()) {
                acc += fabs(d[j] - gd) / gd;
                ++cnt;
            }
        }
        s_sum[tid] = acc;
        s_cnt[tid] = cnt;
        __syncthreads();
        for (int step = WDST_BLOCK >> 1; step > 0; step >>= 1) {
            if (tid < step) {
                s_sum[tid] += s_sum[tid + step];
                s_cnt[tid] += s_cnt[tid + step];
            }
            __syncthreads();
        }
        if (tid == 0) {
            a.sum[r] = s_sum[0];
            a.count[r] = s_cnt[0];
        }
        __syncthreads();
    }
}

int64_t padded_sources(int64_t src_count) { return (src_count + K - 1) / K * K; }

}  // namespace

extern "C" {

int64_t sympa_graph_weighted_workspace_bytes(int64_t num_nodes, int64_t src_count) {
    if (num_nodes <= 0 || src_count <= 0) return 0;
    const int64_t padded = padded_sources(src_count);
    if (padded > INT64_MAX / 8 / (num_nodes + 1)) return INT64_MAX;        // no such buffer: every call is then refused
    return padded * (num_nodes + 1) * 8;
}

int sympa_graph_weighted_rows(const int64_t* rowptr, const int32_t* cols, const double* weights, int64_t num_nodes,
                              int64_t num_entries, int64_t src_begin, int64_t src_count, double* out, int64_t row_stride,
                              void* workspace, int64_t workspace_bytes, int32_t* status, void* stream) {
    if (num_nodes <= 0 || num_nodes > (int64_t)0x7fffffff)
        return fail(SYMPA_ERR_BAD_ARG, "graph weighted rows: num_nodes outside [1, 2^31-1]");
    if (num_entries < 0) return fail(SYMPA_ERR_BAD_ARG, "graph weighted rows: negative num_entries");
    if (src_begin < 0 || src_count < 0 || src_begin + src_count > num_nodes)
        return fail(SYMPA_ERR_BAD_ARG, "graph weighted rows: source block outside [0, num_nodes)");
    if (row_stride < num_nodes) return fail(SYMPA_ERR_BAD_ARG, "graph weighted rows: row_stride smaller than num_nodes");
    if (rowptr == nullptr || ((cols == nullptr || weights == nullptr) && num_entries > 0))
        return fail(SYMPA_ERR_BAD_ARG, "graph weighted rows: null CSR buffer");
    if (src_count == 0) return 0;
    if (out == nullptr) return fail(SYMPA_ERR_BAD_ARG, "graph weighted rows: null output");
    const int64_t need = sympa_graph_weighted_workspace_bytes(num_nodes, src_count);
    if (need == INT64_MAX || workspace == nullptr || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7))
        return fail(SYMPA_ERR_BAD_ARG, "graph weighted rows: workspace missing, too small or not 8-byte aligned");
    SsspArgs a;
    std::memset(&a, 0, sizeof(a));
    a.rowptr = rowptr;
    a.cols = cols;
    a.weights = weights;
    a.N = num_nodes;
    a.E = num_entries;
    a.src_begin = src_begin;
    a.src_count = src_count;
    a.row_stride = row_stride;
    a.out = out;
    a.ws = reinterpret_cast<double*>(workspace);
    a.sweeps = reinterpret_cast<int64_t*>(workspace) + padded_sources(src_count) * num_nodes;
    a.status = status;
    const unsigned grid = (unsigned)((src_count + K - 1) / K);
    hipLaunchKernelGGL(graph_sssp_kernel, dim3(grid), dim3(SSSP_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail((int)e, hipGetErrorString(e));
    return 0;
}

int sympa_graph_weighted_distortion_rows(const double* dist, int64_t ld_dist, const double* gdist, int64_t ld_g,
                                         int64_t row_begin, int64_t row_count, int64_t num_nodes, double* row_sum,
                                         int64_t* row_pairs, void* stream) {
    if (num_nodes <= 0) return fail(SYMPA_ERR_BAD_ARG, "graph weighted distortion: num_nodes must be positive");
    if (row_begin < 0 || row_count < 0 || row_begin + row_count > num_nodes)
        return fail(SYMPA_ERR_BAD_ARG, "graph weighted distortion: row block outside the matrix");
    if (ld_dist < num_nodes || ld_g < num_nodes)
        return fail(SYMPA_ERR_BAD_ARG, "graph weighted distortion: leading dimension smaller than num_nodes");
    if (row_count == 0) return 0;
    if (dist == nullptr || gdist == nullptr || row_sum == nullptr || row_pairs == nullptr)
        return fail(SYMPA_ERR_BAD_ARG, "graph weighted distortion: null buffer");
    WeightedDistortionArgs a;
    std::memset(&a, 0, sizeof(a));
    a.dist = dist;
    a.gdist = gdist;
    a.rows = row_count;
    a.ld_dist = ld_dist;
    a.ld_g = ld_g;
    a.row_begin = row_begin;
    a.N = num_nodes;
    a.sum = row_sum;
    a.count = row_pairs;
    const unsigned grid = (unsigned)(row_count < 65536 ? row_count : 65536);
    hipLaunchKernelGGL(graph_weighted_distortion_kernel, dim3(grid), dim3(WDST_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail((int)e, hipGetErrorString(e));
    return 0;
}

}  // extern "C"
