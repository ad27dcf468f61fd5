// dn_implicit.hip -- implicit (backward-Euler) diffusion, diffusion_method = 'implicit_sparse' (ops.implicit_solve): for every mesh b of a batch
// and every channel c the sparse, symmetric, positive definite system
//
//     (diag(m_b) + t_c L_b) x_bc = rhs_bc            rhs = m (.) u forward, d_x backward
//
// solved by Jacobi-preconditioned conjugate gradients, all B C systems side by side.  L is CSR (int32 rowptr / col, fp32 val) over the
// concatenated vertex axis, block diagonal over the meshes; the blocks u, x are fp32 row-major [v_total][C].
//
// Shape: the access pattern of cheb_step_kernel (dn_eigen.hip).  The 64 lanes of a wave are 64 consecutive channels, a wave owns one row at a
// time, so a neighbour's row segment is ONE contiguous 512-byte read and rowptr / col / val are the same for every lane (wave-uniform: scalar
// loads).  256 threads = 4 waves; a workgroup owns one tile of <= IM_ROWS consecutive rows of ONE mesh (the tile table is built from the mesh
// sizes, tiles never straddle meshes; wave w takes rows w, w + 4, ... of the tile) and one 64-channel column tile (blockIdx.y; lanes past C
// read and write nothing).  Because lanes are channels a per-channel dot product needs no cross-lane step: each lane sums its own rows in row
// order, the four waves combine through LDS in wave order, and the workgroup writes ONE partial per (tile, channel).  A mesh's partials are
// summed in tile order by im_mesh_sum (four contiguous runs of tiles, combined in run order): every sum has one fixed order, nothing is
// atomic, and two runs give the same bits.
//
// Launches.  init: im_init_kernel (diag(L), x0, r, p, partials) + im_reduce_kernel.  One iteration, FOUR launches:
//   1. im_product_kernel   q = m p + t (L p), partial of p.q                           (gathers the neighbours' p)
//   2. im_update_kernel    alpha = rz / sum(p.q) -- every workgroup re-reduces ITS mesh's partials, no launch for it --
//                          x += alpha p, r -= alpha q, partials of r.z and r.r with z = r / d
//   3. im_reduce_kernel    one workgroup per (mesh, column tile): rz, rr, beta, the iteration count, the done flag
//   4. im_pupdate_kernel   p = r / d + beta p      (a pass of its own: launch 1 of the next iteration gathers the neighbours' p)
// Two reductions per iteration are what plain CG has; a launch for the first too would make five.  No workgroup reads a word that another
// workgroup of the same launch writes (the scalars alpha needs were written one launch earlier), so nothing is double-buffered.
// A call of dn_implicit_iterate_f32 ends with im_count_kernel (the systems not yet done -> one int32 for the host).
//
// Arithmetic: x, r, p, q, the partials and the scalars are fp64; val, mass, time, u are read as fp32 and widened on load; z = r / d with
// d = m + t diag(L) is recomputed where it is needed (diag(L) is kept per row, not d per element).  A system (mesh, channel) is done when
// sqrt(r.r) <= rtol sqrt(b.b), both over that mesh's rows; a done system is FROZEN: its lanes skip every store, so further iterations change
// no bit of its x, r, p and no 0 / 0 is formed.  The scalars are per (mesh, channel): a NaN or inf stays in the system it came from.
#include "dn_common.h"
#include "../../include/diffnet_hip.h"

#define IM_WAVES 4
#define IM_RPW 16                        /* rows per wave */
#define IM_ROWS (IM_WAVES * IM_RPW)      /* rows per tile: dn_implicit_rows_per_tile() */
#define IM_CHUNK 8                       /* entries gathered per step */

namespace {
enum { IM_PQ = 0, IM_RZ = 1, IM_RR = 2, IM_BB = 3, IM_NPART = 4 };                 // partial slots [slot][tile][C]
enum { IM_S_RZ = 0, IM_S_RR = 1, IM_S_BB = 2, IM_S_THR = 3, IM_S_BETA = 4, IM_NSC = 5 };   // scalar slots [slot][mesh][C]

struct ImArgs {
    const int* rowptr; const int* col; const float* val; const float* mass; const float* time;
    const DnTile* tiles; const int* mesh_off;    // mesh_off [n_mesh + 1]: the tiles of mesh b are [mesh_off[b], mesh_off[b + 1])
    int n_tiles, n_mesh, v_total, C;
    double *x, *r, *p, *q;                       // [v_total][C]
    double* diag;                                // [v_total] diag(L)
    double* part;                                // [IM_NPART][n_tiles][C]
    double* sc;                                  // [IM_NSC][n_mesh][C]
    int* done; int* iters;                       // [n_mesh][C]
    // init
    const float* rhs; const float* x0; int rhs_mass; double rtol;
    // finish
    float* out; int out_mass; int* o_iters; double* o_res;
    // L x dot
    const float* xf; float* d_time;
    int init;                                    // im_reduce_kernel: 1 = after im_init_kernel
};

__device__ __forceinline__ int im_uniform(int v) {
#ifdef DN_EMULATE
    return v;
#else
    return __builtin_amdgcn_readfirstlane(v);
#endif
}

struct ImWork { long long tile; int row0, nrows, mesh, t0, t1; };

__device__ __forceinline__ void im_mesh_tiles(const ImArgs& a, int mesh, int& t0, int& t1) {
    t0 = a.mesh_off[mesh]; t1 = a.mesh_off[mesh + 1];
    t0 = t0 < 0 ? 0 : (t0 > a.n_tiles ? a.n_tiles : t0);           // a table that lies reads no partial outside the workspace
    t1 = t1 < t0 ? t0 : (t1 > a.n_tiles ? a.n_tiles : t1);
}

// The tile of this workgroup (grid.x walks the tiles XCD by XCD, as the gathers do); false: none, and every thread of the workgroup leaves
// together.  A tile is cut to the rows that exist, whatever the table says: nothing outside [0, v_total) is read or written.
__device__ __forceinline__ bool im_work(const ImArgs& a, ImWork& w) {
    const int per_xcd = (int)(gridDim.x >> 3);
    w.tile = (long long)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (w.tile >= a.n_tiles) return false;
    const DnTile t = a.tiles[w.tile];
    w.row0 = im_uniform(t.row0); w.nrows = im_uniform(t.nrows); w.mesh = im_uniform(t.mesh);
    if (w.row0 < 0 || w.row0 >= a.v_total || w.nrows < 1 || w.mesh < 0 || w.mesh >= a.n_mesh) return false;
    if (w.nrows > IM_ROWS) w.nrows = IM_ROWS;
    if (w.nrows > a.v_total - w.row0) w.nrows = a.v_total - w.row0;
    im_mesh_tiles(a, w.mesh, w.t0, w.t1);
    return true;
}

// the four waves' lane sums -> one partial per channel, in wave order (every thread of the workgroup calls it)
__device__ __forceinline__ void im_tile_partial(double v, double* dst, bool in_c, long long c, int wave, int lane, double (*sh)[64]) {
    sh[wave][lane] = v;
    __syncthreads();
    if (wave == 0 && in_c) dst[c] = ((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane];
    __syncthreads();
}

// sum of a mesh's partials of one slot for this lane's channel, the same bits in every wave and workgroup: wave w sums the w-th of four
// contiguous runs of tiles in tile order, the runs are added in run order (every thread of the workgroup calls it)
__device__ __forceinline__ double im_mesh_sum(const double* slot, int t0, int t1, int C, bool in_c, long long c, int wave, int lane, double (*sh)[64]) {
    const int run = (t1 - t0 + IM_WAVES - 1) / IM_WAVES;
    const int b = t0 + wave * run, e = b + run < t1 ? b + run : t1;
    double s = 0.0;
    if (in_c) for (int t = b; t < e; ++t) s += slot[(size_t)t * C + (size_t)c];
    sh[wave][lane] = s;
    __syncthreads();
    const double tot = ((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane];
    __syncthreads();
    return tot;
}

// sum_p val[p] * src[col[p]][c] (* 1 / mass[col[p]] with INV) over one row, one fma per entry in CSR order; diag: the sum of the entries on the diagonal
template <typename T, bool INV, bool DIAG>
__device__ __forceinline__ double im_row(const ImArgs& a, const T* DN_RESTRICT src, long long v, long long c, bool live, double* diag) {
    const int beg = a.rowptr[v], end = a.rowptr[v + 1];
    double acc = 0.0, dg = 0.0;
    for (int j0 = beg; j0 < end; j0 += IM_CHUNK) {                // an empty row: acc stays 0
        double yv[IM_CHUNK], sv[IM_CHUNK];
#pragma unroll
        for (int u = 0; u < IM_CHUNK; ++u) {                      // branch-free reads: the slots past the row's end repeat its last entry
            const int j = j0 + u < end ? j0 + u : end - 1;
            const int cj = a.col[j];
            sv[u] = (double)a.val[j];
            yv[u] = live ? (double)src[(size_t)cj * a.C + (size_t)c] : 0.0;
            if (INV) yv[u] = yv[u] / (double)a.mass[cj];
            if (DIAG) dg = (j0 + u < end && cj == v) ? dg + sv[u] : dg;
        }
#pragma unroll
        for (int u = 0; u < IM_CHUNK; ++u)
            acc = j0 + u < end ? fma(sv[u], yv[u], acc) : acc;    // uniform condition: a repeated entry is not summed
    }
    if (DIAG) *diag = dg;
    return acc;
}

#define IM_PROLOGUE                                                                      \
    __shared__ double sh[IM_WAVES][64];                                                  \
    const int lane = threadIdx.x & 63;                                                   \
    const int wave = im_uniform((int)(threadIdx.x >> 6));                                \
    const long long c = (long long)blockIdx.y * 64 + lane;                               \
    const bool in_c = c < a.C

// grid (tiles rounded up to a multiple of 8, 64-channel tiles).  x = x0 (NULL: rhs, or rhs / m when rhs is not u), r = b - A x, p = r / d,
// diag(L) by scanning the row for col == i (an empty row gives d = m), partials of r.z, r.r and b.b
template <bool X0, bool INV>   // INV: x0 = rhs / m (no x0 given and rhs is b itself)
__global__ __launch_bounds__(256) void im_init_kernel(ImArgs a) {
    IM_PROLOGUE;
    ImWork w;
    if (!im_work(a, w)) return;
    const double t = in_c ? (double)a.time[c] : 0.0;
    double s_rz = 0.0, s_rr = 0.0, s_bb = 0.0;
    for (int k = wave; k < w.nrows; k += IM_WAVES) {              // uniform per wave
        const long long v = (long long)w.row0 + k;
        const double m = (double)a.mass[v];
        double dg;
        const double lx = im_row<float, INV, true>(a, X0 ? a.x0 : a.rhs, v, c, in_c, &dg);
        if (in_c) {
            const size_t at = (size_t)v * a.C + (size_t)c;
            const double u = (double)a.rhs[at];
            const double b = a.rhs_mass ? m * u : u;
            const double xv = X0 ? (double)a.x0[at] : (INV ? u / m : u);
            const double r = b - fma(t, lx, m * xv);
            const double z = r / (m + t * dg);
            a.x[at] = xv; a.r[at] = r; a.p[at] = z;
            s_rz = fma(r, z, s_rz); s_rr = fma(r, r, s_rr); s_bb = fma(b, b, s_bb);
        }
        if (lane == 0 && blockIdx.y == 0) a.diag[v] = dg;
    }
    const size_t nt = (size_t)a.n_tiles * a.C, at = (size_t)w.tile * a.C;
    im_tile_partial(s_rz, a.part + IM_RZ * nt + at, in_c, c, wave, lane, sh);
    im_tile_partial(s_rr, a.part + IM_RR * nt + at, in_c, c, wave, lane, sh);
    im_tile_partial(s_bb, a.part + IM_BB * nt + at, in_c, c, wave, lane, sh);
}

// LXDOT false: q = m p + t (L p) and the tile's partial of p.q (done systems skipped).  LXDOT true: the partial of g.(L x) with x the fp32
// block a.xf and g the fp64 solution a.x; nothing but the partial is stored
template <bool LXDOT>
__global__ __launch_bounds__(256) void im_product_kernel(ImArgs a) {
    IM_PROLOGUE;
    ImWork w;
    if (!im_work(a, w)) return;
    const bool live = in_c && (LXDOT || !a.done[(size_t)w.mesh * a.C + (size_t)c]);
    const double t = live && !LXDOT ? (double)a.time[c] : 0.0;
    double s = 0.0;
    for (int k = wave; k < w.nrows; k += IM_WAVES) {
        const long long v = (long long)w.row0 + k;
        const size_t at = (size_t)v * a.C + (size_t)c;
        if (LXDOT) {
            const double lx = im_row<float, false, false>(a, a.xf, v, c, live, nullptr);
            if (live) s = fma(a.x[at], lx, s);
        } else {
            const double lp = im_row<double, false, false>(a, a.p, v, c, live, nullptr);
            if (live) {
                const double pv = a.p[at];
                const double qv = fma(t, lp, (double)a.mass[v] * pv);
                a.q[at] = qv;
                s = fma(pv, qv, s);
            }
        }
    }
    im_tile_partial(s, a.part + (size_t)IM_PQ * a.n_tiles * a.C + (size_t)w.tile * a.C, in_c, c, wave, lane, sh);
}

// x += alpha p, r -= alpha q; partials of r.z (z = r / d) and r.r.  alpha = rz / (p.q): the mesh's partials of p.q re-reduced here
__global__ __launch_bounds__(256) void im_update_kernel(ImArgs a) {
    IM_PROLOGUE;
    ImWork w;
    if (!im_work(a, w)) return;
    const size_t nt = (size_t)a.n_tiles * a.C, mc = (size_t)w.mesh * a.C + (size_t)c;
    const double pq = im_mesh_sum(a.part + IM_PQ * nt, w.t0, w.t1, a.C, in_c, c, wave, lane, sh);
    const bool live = in_c && !a.done[mc];
    const double alpha = live ? a.sc[(size_t)IM_S_RZ * a.n_mesh * a.C + mc] / pq : 0.0;
    const double t = live ? (double)a.time[c] : 0.0;
    double s_rz = 0.0, s_rr = 0.0;
    for (int k = wave; k < w.nrows; k += IM_WAVES) {
        const long long v = (long long)w.row0 + k;
        if (live) {
            const size_t at = (size_t)v * a.C + (size_t)c;
            const double d = (double)a.mass[v] + t * a.diag[v];
            const double pv = a.p[at], qv = a.q[at];
            const double xv = fma(alpha, pv, a.x[at]), r = fma(-alpha, qv, a.r[at]);
            a.x[at] = xv; a.r[at] = r;
            s_rz = fma(r, r / d, s_rz); s_rr = fma(r, r, s_rr);
        }
    }
    im_tile_partial(s_rz, a.part + IM_RZ * nt + (size_t)w.tile * a.C, in_c, c, wave, lane, sh);
    im_tile_partial(s_rr, a.part + IM_RR * nt + (size_t)w.tile * a.C, in_c, c, wave, lane, sh);
}

// grid (n_mesh, 64-channel tiles): the scalars of one mesh.  After init: rz, rr, bb, the threshold rtol sqrt(bb), iterations = 0, done.
// After an update: beta = rz' / rz, rz, rr, iterations + 1, done -- for the systems that were not done; a done system keeps every word
__global__ __launch_bounds__(256) void im_reduce_kernel(ImArgs a) {
    IM_PROLOGUE;
    const int mesh = (int)blockIdx.x;
    int t0, t1;
    im_mesh_tiles(a, mesh, t0, t1);
    const size_t nt = (size_t)a.n_tiles * a.C, ns = (size_t)a.n_mesh * a.C, mc = (size_t)mesh * a.C + (size_t)c;
    const double rz = im_mesh_sum(a.part + IM_RZ * nt, t0, t1, a.C, in_c, c, wave, lane, sh);
    const double rr = im_mesh_sum(a.part + IM_RR * nt, t0, t1, a.C, in_c, c, wave, lane, sh);
    double bb = 0.0;
    if (a.init) bb = im_mesh_sum(a.part + IM_BB * nt, t0, t1, a.C, in_c, c, wave, lane, sh);
    if (wave != 0 || !in_c) return;                               // (behind the last barrier)
    if (a.init) {
        const double thr = a.rtol * sqrt(bb);
        a.sc[IM_S_RZ * ns + mc] = rz; a.sc[IM_S_RR * ns + mc] = rr; a.sc[IM_S_BB * ns + mc] = bb; a.sc[IM_S_THR * ns + mc] = thr;
        a.sc[IM_S_BETA * ns + mc] = 0.0;
        a.iters[mc] = 0;
        a.done[mc] = sqrt(rr) <= thr ? 1 : 0;                     // (NaN: never done)
    } else if (!a.done[mc]) {
        a.sc[IM_S_BETA * ns + mc] = rz / a.sc[IM_S_RZ * ns + mc];
        a.sc[IM_S_RZ * ns + mc] = rz; a.sc[IM_S_RR * ns + mc] = rr;
        a.iters[mc] += 1;
        a.done[mc] = sqrt(rr) <= a.sc[IM_S_THR * ns + mc] ? 1 : 0;
    }
}

// p = r / d + beta p for the systems not done (no barrier: the lanes without work leave)
__global__ __launch_bounds__(256) void im_pupdate_kernel(ImArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = im_uniform((int)(threadIdx.x >> 6));
    const long long c = (long long)blockIdx.y * 64 + lane;
    ImWork w;
    if (!im_work(a, w)) return;
    if (c >= a.C || a.done[(size_t)w.mesh * a.C + (size_t)c]) return;
    const double beta = a.sc[(size_t)IM_S_BETA * a.n_mesh * a.C + (size_t)w.mesh * a.C + (size_t)c];
    const double t = (double)a.time[c];
    for (int k = wave; k < w.nrows; k += IM_WAVES) {
        const long long v = (long long)w.row0 + k;
        const size_t at = (size_t)v * a.C + (size_t)c;
        a.p[at] = fma(beta, a.p[at], a.r[at] / ((double)a.mass[v] + t * a.diag[v]));
    }
}

// one workgroup: *unfinished = the systems (mesh, channel) not done (integer adds in LDS: any order gives the same count)
__global__ __launch_bounds__(256) void im_count_kernel(const int* done, long long n, int* unfinished) {
    __shared__ int total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    int mine = 0;
    for (long long i = threadIdx.x; i < n; i += 256) mine += done[i] ? 0 : 1;
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    if (threadIdx.x == 0) *unfinished = total;
}

// out = fp32(x) (out_mass: fp32(m x)); the workgroup of a mesh's first tile writes that mesh's iterations and sqrt(rr) / sqrt(bb)
__global__ __launch_bounds__(256) void im_finish_kernel(ImArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = im_uniform((int)(threadIdx.x >> 6));
    const long long c = (long long)blockIdx.y * 64 + lane;
    ImWork w;
    if (!im_work(a, w)) return;
    if (c >= a.C) return;
    for (int k = wave; k < w.nrows; k += IM_WAVES) {
        const long long v = (long long)w.row0 + k;
        const size_t at = (size_t)v * a.C + (size_t)c;
        a.out[at] = (float)(a.out_mass ? (double)a.mass[v] * a.x[at] : a.x[at]);
    }
    if (w.tile == w.t0 && wave == 0) {
        const size_t ns = (size_t)a.n_mesh * a.C, mc = (size_t)w.mesh * a.C + (size_t)c;
        if (a.o_iters) a.o_iters[mc] = a.iters[mc];
        if (a.o_res) {
            const double rr = a.sc[IM_S_RR * ns + mc];
            a.o_res[mc] = rr == 0.0 ? 0.0 : sqrt(rr) / sqrt(a.sc[IM_S_BB * ns + mc]);
        }
    }
}

// grid (64-channel tiles): d_time[c] = - sum over meshes, in mesh order, of the mesh's partials of g.(L x)
__global__ __launch_bounds__(256) void im_dtime_kernel(ImArgs a) {
    __shared__ double sh[IM_WAVES][64];
    const int lane = threadIdx.x & 63;
    const int wave = im_uniform((int)(threadIdx.x >> 6));
    const long long c = (long long)blockIdx.x * 64 + lane;
    const bool in_c = c < a.C;
    double s = 0.0;
    for (int mesh = 0; mesh < a.n_mesh; ++mesh) {
        int t0, t1;
        im_mesh_tiles(a, mesh, t0, t1);
        s += im_mesh_sum(a.part + (size_t)IM_PQ * a.n_tiles * a.C, t0, t1, a.C, in_c, c, wave, lane, sh);
    }
    if (wave == 0 && in_c) a.d_time[c] = (float)(-s);
}

size_t im_align(size_t n) { return (n + 15) & ~(size_t)15; }

// the workspace's pieces in a; returns the bytes they take from a 16-byte aligned base
size_t im_carve(char* base, ImArgs& a) {
    const size_t vc = (size_t)a.v_total * a.C, mc = (size_t)a.n_mesh * a.C;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += im_align(bytes); return p; };
    a.x = (double*)take(vc * 8); a.r = (double*)take(vc * 8); a.p = (double*)take(vc * 8); a.q = (double*)take(vc * 8);
    a.diag = (double*)take((size_t)a.v_total * 8);
    a.part = (double*)take((size_t)IM_NPART * a.n_tiles * a.C * 8);
    a.sc = (double*)take((size_t)IM_NSC * mc * 8);
    a.done = (int*)take(mc * 4); a.iters = (int*)take(mc * 4);
    return off + 16;                                              // (+ 16: the base is rounded up to 16 bytes)
}

// 0: the sizes describe a problem the kernels take
int im_sizes_ok(int n_tiles, int n_mesh, int v_total, int C) {
    if (n_tiles < 0 || n_mesh < 0 || v_total < 0 || C < 0) return 0;
    if (((long long)C + 63) / 64 > 65535) return 0;                                   /* grid.y */
    if ((long long)n_tiles * IM_ROWS < (long long)v_total || n_tiles > v_total) return 0;   /* the table cannot cover v_total / holds an empty tile */
    if (n_mesh > n_tiles || (v_total > 0 && n_mesh < 1)) return 0;
    return 1;
}

// fills the shared fields; non-zero: refused
int im_setup(ImArgs& a, const int32_t* rowptr, const int32_t* col, const float* val, const float* mass, const float* time, const int32_t* tiles,
             int n_tiles, const int32_t* mesh_off, int n_mesh, int v_total, int C, void* ws, size_t ws_bytes) {
    if (!im_sizes_ok(n_tiles, n_mesh, v_total, C)) return 1;                          /* hipErrorInvalidValue */
    a = ImArgs{};
    a.rowptr = rowptr; a.col = col; a.val = val; a.mass = mass; a.time = time;
    a.tiles = reinterpret_cast<const DnTile*>(tiles); a.mesh_off = mesh_off;
    a.n_tiles = n_tiles; a.n_mesh = n_mesh; a.v_total = v_total; a.C = C;
    if (v_total == 0 || C == 0) return 0;
    if (!tiles || !mesh_off || !ws) return 1;
    char* base = reinterpret_cast<char*>(((uintptr_t)ws + 15) & ~(uintptr_t)15);
    if (im_carve(base, a) > ws_bytes) return 1;
    return 0;
}

dim3 im_grid(const ImArgs& a) { return dim3((unsigned)(((long long)a.n_tiles + 7) / 8 * 8), (unsigned)((a.C + 63) / 64), 1); }
dim3 im_mesh_grid(const ImArgs& a) { return dim3((unsigned)a.n_mesh, (unsigned)((a.C + 63) / 64), 1); }
}  // namespace

extern "C" {

int dn_implicit_rows_per_tile(void) { return IM_ROWS; }

size_t dn_implicit_workspace_bytes(int v_total, int C, int n_tiles, int n_mesh) {
    if (!im_sizes_ok(n_tiles, n_mesh, v_total, C)) return 0;
    ImArgs a{};
    a.n_tiles = n_tiles; a.n_mesh = n_mesh; a.v_total = v_total; a.C = C;
    return im_carve(nullptr, a);
}

int dn_implicit_init_f32(const int32_t* rowptr, const int32_t* col, const float* val, const float* mass, const float* time, const int32_t* tiles,
                         int n_tiles, const int32_t* mesh_tile_off, int n_mesh, int v_total, int C, const float* rhs, int rhs_mass, const float* x0,
                         double rtol, void* ws, size_t ws_bytes, void* stream) {
    ImArgs a;
    if (im_setup(a, rowptr, col, val, mass, time, tiles, n_tiles, mesh_tile_off, n_mesh, v_total, C, ws, ws_bytes)) return 1;
    if (!(rtol >= 0.0)) return 1;
    if (v_total == 0 || C == 0) return 0;
    if (!rowptr || !col || !val || !mass || !time || !rhs) return 1;
    a.rhs = rhs; a.x0 = x0; a.rhs_mass = rhs_mass; a.rtol = rtol; a.init = 1;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid = im_grid(a), blk(256, 1, 1);
    if (x0) DN_LAUNCH((im_init_kernel<true, false>), grid, blk, 0, st, a);
    else if (rhs_mass) DN_LAUNCH((im_init_kernel<false, false>), grid, blk, 0, st, a);
    else DN_LAUNCH((im_init_kernel<false, true>), grid, blk, 0, st, a);
    DN_LAUNCH(im_reduce_kernel, im_mesh_grid(a), blk, 0, st, a);
    return (int)hipGetLastError();
}

int dn_implicit_iterate_f32(const int32_t* rowptr, const int32_t* col, const float* val, const float* mass, const float* time, const int32_t* tiles,
                            int n_tiles, const int32_t* mesh_tile_off, int n_mesh, int v_total, int C, int n_iter, int32_t* unfinished, void* ws,
                            size_t ws_bytes, void* stream) {
    ImArgs a;
    if (im_setup(a, rowptr, col, val, mass, time, tiles, n_tiles, mesh_tile_off, n_mesh, v_total, C, ws, ws_bytes)) return 1;
    if (n_iter < 0 || !unfinished) return 1;
    if (v_total == 0 || C == 0) return 0;
    if (!rowptr || !col || !val || !mass || !time) return 1;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid = im_grid(a), blk(256, 1, 1);
    for (int it = 0; it < n_iter; ++it) {
        DN_LAUNCH(im_product_kernel<false>, grid, blk, 0, st, a);
        DN_LAUNCH(im_update_kernel, grid, blk, 0, st, a);
        DN_LAUNCH(im_reduce_kernel, im_mesh_grid(a), blk, 0, st, a);
        DN_LAUNCH(im_pupdate_kernel, grid, blk, 0, st, a);
    }
    DN_LAUNCH(im_count_kernel, dim3(1, 1, 1), blk, 0, st, a.done, (long long)n_mesh * C, unfinished);
    return (int)hipGetLastError();
}

int dn_implicit_finish_f32(const float* mass, const int32_t* tiles, int n_tiles, const int32_t* mesh_tile_off, int n_mesh, int v_total, int C,
                           int out_mass, float* out, int32_t* iterations, double* residual, void* ws, size_t ws_bytes, void* stream) {
    ImArgs a;
    if (im_setup(a, nullptr, nullptr, nullptr, mass, nullptr, tiles, n_tiles, mesh_tile_off, n_mesh, v_total, C, ws, ws_bytes)) return 1;
    if (v_total == 0 || C == 0) return 0;
    if (!out || (out_mass && !mass)) return 1;
    a.out = out; a.out_mass = out_mass; a.o_iters = iterations; a.o_res = residual;
    DN_LAUNCH(im_finish_kernel, im_grid(a), dim3(256, 1, 1), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int dn_implicit_lx_dot_f32(const int32_t* rowptr, const int32_t* col, const float* val, const int32_t* tiles, int n_tiles,
                           const int32_t* mesh_tile_off, int n_mesh, int v_total, int C, const float* x, float* d_time, void* ws, size_t ws_bytes,
                           void* stream) {
    ImArgs a;
    if (im_setup(a, rowptr, col, val, nullptr, nullptr, tiles, n_tiles, mesh_tile_off, n_mesh, v_total, C, ws, ws_bytes)) return 1;
    if (C > 0 && !d_time) return 1;
    if (C == 0) return 0;
    if (v_total > 0 && (!rowptr || !col || !val || !x)) return 1;
    a.xf = x; a.d_time = d_time;
    const hipStream_t st = (hipStream_t)stream;
    if (v_total > 0) DN_LAUNCH(im_product_kernel<true>, im_grid(a), dim3(256, 1, 1), 0, st, a);
    DN_LAUNCH(im_dtime_kernel, dim3((unsigned)((C + 63) / 64), 1, 1), dim3(256, 1, 1), 0, st, a);
    return (int)hipGetLastError();
}

}  // extern "C"
