// C-ABI sympa_graph_hop_rows / sympa_graph_hops_workspace_bytes / sympa_graph_distortion_rows: hop distances (unweighted shortest
// paths) from a block of source nodes to every node of a symmetric CSR graph, and the distortion of a block of manifold
// distance rows against them.  The device counterpart of the APSP the reference runs in preprocess.py:101-126.
//
// Level-synchronous, bit-parallel, pull-based multi-source BFS.  One workgroup owns ONE word of 64 consecutive sources for the
// whole search; bit b of a node's word stands for source src_begin + 64 word + b.  Three node planes per word live in the
// caller's workspace, word-major ([word][plane][N] uint64): seen, and two frontiers that swap roles every level.  At level L a
// lane that owns node v ORs the frontier words of v's neighbours, masks the result with ~seen[v] and, for every bit that is
// new, stores L to out[bit][v].  The wave walks the distinct new bits together, so for a fixed bit adjacent lanes store to
// adjacent addresses.  Levels are separated by workgroup barriers only (the block-wide OR that ends the loop is one of them):
// no inter-workgroup synchronisation, no cooperative launch, no host round trip per level, and no atomics on the search path
// (the status word of a malformed CSR is the one exception).  The level loop is bounded by N - 1 in its header.
// Every element of the block is written exactly once: 0 on the diagonal at the start, the level when a node is discovered,
// -1 after the loop for the bits never seen.  Hop distances are unique, so the result does not depend on the blocking.
#include "siegel_common.hpp"

namespace {
using namespace sympa_hip;

constexpr int BFS_BLOCK = 1024;
constexpr int DST_BLOCK = 256;
typedef unsigned long long u64;

struct BfsArgs {
    const int64_t* rowptr;
    const int32_t* cols;
    int64_t N, E, src_begin, src_count, row_stride;
    int32_t* out;
    u64* ws;
    int32_t* status;
};

// stores `value` to out[bit][v] for every set bit of `bits`; the wave takes one distinct bit per trip
__device__ __forceinline__ void store_bits(u64 bits, int32_t* out_v, const int64_t row_stride, const int32_t value) {
    while (true) {
        const u64 active = __ballot(bits != 0);
        if (active == 0) break;
        const int leader = __ffsll((long long)active) - 1;
        const u64 lead_bits = __shfl(bits, leader);
        const int b = __ffsll((long long)lead_bits) - 1;
        const u64 m = 1ull << b;
        if (bits & m) {
            out_v[(int64_t)b * row_stride] = value;
            bits &= ~m;
        }
    }
}

__global__ __launch_bounds__(BFS_BLOCK) void graph_bfs_kernel(const BfsArgs a) {
    const int tid = threadIdx.x;
    const int64_t N = a.N;
    const int64_t word = blockIdx.x;
    const int64_t first = a.src_begin + word * 64;                       // source of bit 0
    const int64_t left = a.src_count - word * 64;
    const int nbits = left < 64 ? (int)left : 64;
    const u64 valid = nbits == 64 ? ~0ull : ((1ull << nbits) - 1);
    u64* seen = a.ws + word * 3 * N;
    u64* cur = seen + N;
    u64* nxt = cur + N;
    int32_t* out = a.out + word * 64 * a.row_stride;

    // workgroup 0 counts the malformed CSR entries once (the search itself only skips them)
    if (blockIdx.x == 0 && a.status != nullptr) {
        int bad = 0;
        for (int64_t v = tid; v < N; v += BFS_BLOCK) {
            const int64_t beg = a.rowptr[v], end = a.rowptr[v + 1];
            if (beg < 0 || end < beg || end > a.E) ++bad;
        }
        for (int64_t e = tid; e < a.E; e += BFS_BLOCK) {
            const int32_t c = a.cols[e];
            if (c < 0 || (int64_t)c >= N) ++bad;
        }
        if (bad) { atomicOr(&a.status[0], sympa::ST_BAD_INDEX); atomicAdd(&a.status[1], bad); }
    }

    for (int64_t v0 = 0; v0 < N; v0 += BFS_BLOCK) {                       // wave-uniform trip count: store_bits shuffles
        const int64_t v = v0 + tid;
        u64 self = 0;
        if (v < N) {
            if (v >= first && v < first + nbits) self = 1ull << (int)(v - first);
            seen[v] = self;
            cur[v] = self;
        }
        store_bits(self, out + (v < N ? v : 0), a.row_stride, 0);
    }
    __syncthreads();

    for (int64_t level = 1; level <= N - 1; ++level) {
        int any = 0;
        for (int64_t v0 = 0; v0 < N; v0 += BFS_BLOCK) {
            const int64_t v = v0 + tid;
            u64 fresh = 0;
            if (v < N) {
                const u64 s = seen[v];
                if (s != valid) {                                         // a node every source has reached pulls nothing
                    int64_t beg = a.rowptr[v], end = a.rowptr[v + 1];
                    beg = beg < 0 ? 0 : beg;
                    end = end > a.E ? a.E : end;
                    u64 f = 0;
                    for (int64_t e = beg; e < end; ++e) {
                        const int32_t c = a.cols[e];
                        if (c >= 0 && (int64_t)c < N) f |= cur[c];
                    }
                    fresh = f & ~s;
                    if (fresh) seen[v] = s | fresh;
                }
                nxt[v] = fresh;
                any |= fresh != 0;
            }
            store_bits(fresh, out + (v < N ? v : 0), a.row_stride, (int32_t)level);
        }
        if (!__syncthreads_or(any)) break;
        u64* t = cur; cur = nxt; nxt = t;
    }

    for (int64_t v0 = 0; v0 < N; v0 += BFS_BLOCK) {
        const int64_t v = v0 + tid;
        const u64 never = v < N ? (~seen[v] & valid) : 0;
        store_bits(never, out + (v < N ? v : 0), a.row_stride, -1);
    }
}

struct DistortionArgs {
    const double* dist;      // [rows, ld_dist]
    const int32_t* hops;     // [rows, ld_hops]
    int64_t rows, ld_dist, ld_hops, row_begin, N;
    double* sum;             // [rows]
    int64_t* count;          // [rows]
};

// Row r (node i = row_begin + r): sum over the columns j > i with hops > 0 of |d - g| / g, and their number.  Lane t adds its
// columns i + 1 + t, i + 1 + t + 256, ... in order and the 256 partial sums meet in a fixed tree: the value of a row depends on
// the row alone, never on the block it arrived in.
__global__ __launch_bounds__(DST_BLOCK) void graph_distortion_kernel(const DistortionArgs a) {
    __shared__ double s_sum[DST_BLOCK];
    __shared__ int64_t s_cnt[DST_BLOCK];
    const int tid = threadIdx.x;
    for (int64_t r = blockIdx.x; r < a.rows; r += gridDim.x) {
        const int64_t i = a.row_begin + r;
        const double* d = a.dist + r * a.ld_dist;
        const int32_t* h = a.hops + r * a.ld_hops;
        double acc = 0.0;
        int64_t cnt = 0;
        for (int64_t j = i + 1 + tid; j < a.N; j += DST_BLOCK) {
            const int32_t g = h[j];
            if (g > 0) {
                const double gd = (double)g;
                acc += fabs(d[j] - gd) / gd;
                ++cnt;
            }
        }
        s_sum[tid] = acc;
        s_cnt[tid] = cnt;
        __syncthreads();
        for (int step = DST_BLOCK >> 1; step > 0; step >>= 1) {
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

}  // namespace

extern "C" {

int64_t sympa_graph_hops_workspace_bytes(int64_t num_nodes, int64_t src_count) {
    if (num_nodes <= 0 || src_count <= 0) return 0;
    return ((src_count + 63) / 64) * 24 * num_nodes;
}

int sympa_graph_hop_rows(const int64_t* rowptr, const int32_t* cols, int64_t num_nodes, int64_t num_entries, int64_t src_begin,
                         int64_t src_count, int32_t* out, int64_t row_stride, void* workspace, int64_t workspace_bytes,
                         int32_t* status, void* stream) {
    if (num_nodes <= 0 || num_nodes > (int64_t)0x7fffffff) return fail(SYMPA_ERR_BAD_ARG, "graph hops: num_nodes outside [1, 2^31-1]");
    if (num_entries < 0) return fail(SYMPA_ERR_BAD_ARG, "graph hops: negative num_entries");
    if (src_begin < 0 || src_count < 0 || src_begin + src_count > num_nodes)
        return fail(SYMPA_ERR_BAD_ARG, "graph hops: source block outside [0, num_nodes)");
    if (row_stride < num_nodes) return fail(SYMPA_ERR_BAD_ARG, "graph hops: row_stride smaller than num_nodes");
    if (rowptr == nullptr || (cols == nullptr && num_entries > 0)) return fail(SYMPA_ERR_BAD_ARG, "graph hops: null CSR buffer");
    if (src_count == 0) return 0;
    if (out == nullptr) return fail(SYMPA_ERR_BAD_ARG, "graph hops: null output");
    const int64_t need = sympa_graph_hops_workspace_bytes(num_nodes, src_count);
    if (workspace == nullptr || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7))
        return fail(SYMPA_ERR_BAD_ARG, "graph hops: workspace missing, too small or not 8-byte aligned");
    BfsArgs a;
    std::memset(&a, 0, sizeof(a));
    a.rowptr = rowptr;
    a.cols = cols;
    a.N = num_nodes;
    a.E = num_entries;
    a.src_begin = src_begin;
    a.src_count = src_count;
    a.row_stride = row_stride;
    a.out = out;
    a.ws = reinterpret_cast<u64*>(workspace);
    a.status = status;
    const unsigned grid = (unsigned)((src_count + 63) / 64);
    hipLaunchKernelGGL(graph_bfs_kernel, dim3(grid), dim3(BFS_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail((int)e, hipGetErrorString(e));
    return 0;
}

int sympa_graph_distortion_rows(const double* dist, int64_t ld_dist, const int32_t* hops, int64_t ld_hops, int64_t row_begin,
                                int64_t row_count, int64_t num_nodes, double* row_sum, int64_t* row_pairs, void* stream) {
    if (num_nodes <= 0) return fail(SYMPA_ERR_BAD_ARG, "graph distortion: num_nodes must be positive");
    if (row_begin < 0 || row_count < 0 || row_begin + row_count > num_nodes)
        return fail(SYMPA_ERR_BAD_ARG, "graph distortion: row block outside the matrix");
    if (ld_dist < num_nodes || ld_hops < num_nodes) return fail(SYMPA_ERR_BAD_ARG, "graph distortion: leading dimension smaller than num_nodes");
    if (row_count == 0) return 0;
    if (dist == nullptr || hops == nullptr || row_sum == nullptr || row_pairs == nullptr)
        return fail(SYMPA_ERR_BAD_ARG, "graph distortion: null buffer");
    DistortionArgs a;
    std::memset(&a, 0, sizeof(a));
    a.dist = dist;
    a.hops = hops;
    a.rows = row_count;
    a.ld_dist = ld_dist;
    a.ld_hops = ld_hops;
    a.row_begin = row_begin;
    a.N = num_nodes;
    a.sum = row_sum;
    a.count = row_pairs;
    const unsigned grid = (unsigned)(row_count < 65536 ? row_count : 65536);
    hipLaunchKernelGGL(graph_distortion_kernel, dim3(grid), dim3(DST_BLOCK), 0, reinterpret_cast<hipStream_t>(stream), a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail((int)e, hipGetErrorString(e));
    return 0;
}

}  // extern "C"
