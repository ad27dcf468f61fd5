// dn_geodesic.hip -- (min, +) relaxation sweeps of a block of distance columns over a CSR graph (ops.minplus_distances; the all-pairs
// mesh distances of geometry.geodesic_label_errors, geometry.py:754-896, on the Steiner-point graph of the mesh).
//
// One sweep is dist[v][s] = min(dist[v][s], min over the arcs (u, w) of row v of dist[u][s] + w) for every node v and source s: the access
// pattern of the CSR gathers of dn_sparse.hip with min in place of +.  The block is node-major, dist[n_nodes][n_src] fp64: the 64 lanes
// of a wave are 64 consecutive sources, a wave owns one node at a time, so a neighbour's row segment is ONE contiguous 512-byte read and the
// row's arcs (col, w) are the same for every lane -- the node index is made wave-uniform, which turns rowptr / col / w into scalar loads.
//
// Arithmetic: exactly one fp64 add per arc, nothing reassociated; min is exact.  fl(x + w) is monotone in x, so the fixed point of the sweeps
// is, for every (v, s), the minimum over the paths s -> v of the left-to-right fp64 sum of the arc lengths -- whatever the order of
// relaxation.  That is what Dijkstra computes, bit for bit.
//
// Sweeps are IN PLACE, one launch per sweep.  A value only ever decreases, every value ever stored is the length of a real path, and an
// aligned 8-byte load or store does not tear, so a lane that reads a neighbour's value while another workgroup lowers it gets the older or
// the newer path length: both are valid upper bounds, and the fixed point is the one above.  Every (v, s) is written by one lane only.  A
// launch boundary makes all earlier stores visible, so a sweep that lowers nothing has read the final values: it certifies the fixed point.
// In place needs half the memory of a ping-pong pair (the block is the large object here: n_nodes x n_src x 8 bytes) and never needs more
// sweeps than Jacobi, usually far fewer.
//
// Shape: 256 threads = 4 waves; a workgroup owns GEO_NODES consecutive nodes (GEO_NPW per wave) of one 64-source group.  blockIdx.x walks the
// node tiles fastest, so the workgroups in flight share a source group: its n_nodes x 512 bytes are what the caches hold.  The arcs of a
// row are taken GEO_CHUNK at a time, branch-free (entries past the row's end repeat its last arc: min is idempotent), so GEO_CHUNK row reads
// are in flight per lane.  No LDS: a row's neighbours are arbitrary nodes and each row segment is read by one wave only.
#include "dn_common.h"
#include "../../include/diffnet_hip.h"

#define GEO_WAVES 4
#define GEO_NPW 4                        /* nodes per wave */
#define GEO_NODES (GEO_WAVES * GEO_NPW)  /* nodes per workgroup: DN_MINPLUS_NODE_TILE */
#define GEO_CHUNK 8                      /* arcs gathered per branch-free step */

namespace {
__device__ __forceinline__ int geo_uniform(int v) {
#ifdef DN_EMULATE
    return v;
#else
    return __builtin_amdgcn_readfirstlane(v);
#endif
}

// grid (node tiles rounded up to a multiple of 8, 64-source groups).  changed: NULL, or the word that is set when a value was lowered.
__global__ __launch_bounds__(256) void minplus_sweep_kernel(const int* DN_RESTRICT rowptr, const int* DN_RESTRICT col, const double* DN_RESTRICT w,
                                                            int n_nodes, double* dist, int n_src, int* changed) {
    const int lane = threadIdx.x & 63;
    const int wave = geo_uniform((int)(threadIdx.x >> 6));
    // every XCD walks a contiguous range of node tiles (block b runs on XCD b % 8), as the CSR gathers do: with neighbouring nodes
    // numbered close to each other (geometry.geodesic_distances uploads the graph in reverse Cuthill-McKee order: a sweep is 1.9x faster
    // at FAUST size than in the builder's order) the rows a tile reads are mostly in the L2 that its neighbours' tiles filled
    const int per_xcd = (int)(gridDim.x >> 3);
    const long long tile = (long long)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    const long long s = (long long)blockIdx.y * 64 + lane;
    const bool live = s < n_src;                                  // ragged n_src: the lanes past the end read and write nothing
    const size_t ld = (size_t)n_src;
    bool lowered = false;
#pragma unroll 1
    for (int r = 0; r < GEO_NPW; ++r) {
        const long long v = tile * GEO_NODES + (long long)wave * GEO_NPW + r;
        if (v >= n_nodes) break;                                  // uniform per wave
        const int beg = rowptr[v], end = rowptr[v + 1];
        if (beg >= end || !live) continue;                        // an empty row keeps its values
        double* mine = dist + (size_t)v * ld + (size_t)s;
        const double old = *mine;
        double best = old;
        for (int j0 = beg; j0 < end; j0 += GEO_CHUNK) {
            double dv[GEO_CHUNK], wv[GEO_CHUNK];
#pragma unroll
            for (int u = 0; u < GEO_CHUNK; ++u) {
                const int j = j0 + u < end ? j0 + u : end - 1;
                wv[u] = w[j];
                dv[u] = dist[(size_t)col[j] * ld + (size_t)s];
            }
#pragma unroll
            for (int u = 0; u < GEO_CHUNK; ++u) {
                const double t = dv[u] + wv[u];
                best = t < best ? t : best;
            }
        }
        if (best < old) {
            *mine = best;
            lowered = true;
        }
    }
    if (changed && lowered) *changed = 1;                         // plain store of the same word by every lane that lowered a value
}
}  // namespace

extern "C" {

int dn_minplus_node_tile(void) { return GEO_NODES; }

int dn_minplus_sweeps_f64(const int32_t* rowptr, const int32_t* col, const double* w, int n_nodes, double* dist, int n_src, int n_sweeps,
                          int32_t* changed, void* stream) {
    if (n_nodes < 0 || n_src < 0 || n_sweeps < 0 || !changed) return 1;   /* hipErrorInvalidValue */
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(changed, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    if (n_nodes == 0 || n_src == 0 || n_sweeps == 0) return 0;
    if (!rowptr || !dist) return 1;
    const long long tiles = ((long long)n_nodes + GEO_NODES - 1) / GEO_NODES;
    const long long groups = ((long long)n_src + 63) / 64;
    if (groups > 65535) return 1;                                         /* grid.y */
    const dim3 grid((unsigned)((tiles + 7) / 8 * 8), (unsigned)groups, 1);
    for (int i = 0; i < n_sweeps; ++i)
        DN_LAUNCH(minplus_sweep_kernel, grid, dim3(256, 1, 1), 0, st, rowptr, col, w, n_nodes, dist, n_src,
                  i == n_sweeps - 1 ? (int*)changed : (int*)nullptr);
    return (int)hipGetLastError();
}

}  // extern "C"
