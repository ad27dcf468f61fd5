// dn_knn_grid.hip -- exact k-nearest-neighbour search for D <= 3 over a dense grid of cells: the bits of dn_knn.hip with work that grows
// with N k instead of N M.
//
// Cells.  The targets are binned into G cells per axis over their bounding cube (edge e = the largest extent, lower corner lo).  G is a host
// function of (M, k, D) (knn_grid_resolve), so every size is known without reading the device; lo and e are read by the kernels from the
// device words the caller computed (box = [lo_0 .. lo_{D-1}, hi_0 .. hi_{D-1}]).  With inv = fl(G / e) and h = fl(e / G) the cell of a
// coordinate x on axis d is
//     u(x) = fl(fl(x - lo_d) * inv),   cell(x) = u >= 0 ? (u < G ? (int)u : G - 1) : 0
// -- monotone in x (a rounded subtraction and a rounded product with a non-negative constant are monotone), and written so that NaN
// (every compare false) and -inf land in cell 0 and +inf in cell G - 1.  An edge that is zero, not finite or below 1e-30 gives inv = h = 0:
// every target falls in cell 0 and the search degenerates to a scan (still exact).  The caller sorts the cell keys (stable), builds the
// cell start table and hands both back; knn_grid_gather_kernel lays the targets out in cell order as (x, y, z, original index).
//
// Search.  One lane per query, the queries taken in cell-sorted order (a wave's 64 queries sit in adjacent cells and share cache lines of
// the sorted targets).  A query visits the cells around its own -- clamped -- cell c in shells of Chebyshev radius r = 0, 1, 2, ...; the
// cells of a shell that are adjacent along x are one contiguous range of the sorted targets.  The squared distance of a pair is the brute
// kernel's arithmetic exactly (q_d - t_d, one fmaf chain over d = 0 .. D-1 from 0, sqrtf on output), the order key is that squared
// distance and equal keys go to the lower ORIGINAL target index; candidates do not arrive in ascending index here, so the insertion
// compares (key, index) as a pair.  (key, index) is a total order: the k best of a row are one set however the candidates are visited,
// which is why the result is bit-identical to dn_knn.hip for every G and every budget.
//
// Closing rule.  After shell r every unseen target t has a cell that differs from c by more than r on some axis d, so it lies beyond a
// face of the cube of cells [c - r, c + r]; a face on the grid's boundary has nothing beyond it and does not count.  Take the upper face
// of axis d, F = c_d + r + 1 <= G - 1.  cell(t_d) >= F means u(t_d) >= F.  With a = fl(t_d - lo_d) >= 0:
//     fl(a inv) >= F  =>  a inv >= F (1 - 2^-24)            (round to nearest)
//     inv = (G / e)(1 + d1), h = (e / G)(1 + d2), fp = fl(F h) = F (e / G)(1 + d2)(1 + d3),  |d_i| <= 2^-24
//     =>  a >= fp (1 - 2^-22), and fp <= e (1 + 2^-23), so  a >= fp - 2^-22 e (1 + ..)
// The kernel knows qa = fl(q_d - lo_d), not q_d - lo_d:  t_d - lo_d >= a (1 - 2^-24) with a <= e (a is a monotone function of t_d <= hi_d),
// and |(q_d - lo_d) - qa| <= 2^-24 |qa| (1 + ..).  Finally g = fl(fp - qa) is off by at most 2^-24 |g| <= 2^-24 (e + |qa|)(1 + ..).  Summed,
//     t_d - q_d >= g - (2^-22 + 2^-24 + 2^-24) e - (2^-24 + 2^-24) |qa| >= g - 2^-21 s,      s = max(e, |qa|)
// (the lower face is the mirror image: u(t_d) < F gives a < fp (1 + 2^-22)).  The kernel subtracts m = 2^-20 s -- twice the sum, which pays
// for the second-order terms and for the rounding of the subtraction itself (whether or not the compiler contracts F h - qa into one fma:
// that only removes a rounding).  lb = g - m is a lower bound of |t_d - q_d| for every target beyond that face; the smallest lb over the
// counting faces bounds every unseen target.  Its fp32 key is at least fl(df^2) with |df| = |fl(q_d - t_d)| >= lb (1 - 2^-24) (the fmaf
// chain of non-negative terms is monotone), so key >= lb^2 (1 - 2^-24)^3 > lb^2 (1 - 2^-22), while the kernel's bound
// B = fl(fl(lb lb)(1 - 2^-20)) <= lb^2 (1 + 2^-24)^2 (1 - 2^-20) is below that.  The query closes when its list holds k entries and the k-th
// key is STRICTLY below B.  lb <= 1e-18 (lb^2 near the subnormals, where the relative bounds above fail) never closes.  Nothing here is
// tuned; being conservative costs a shell, never a neighbour.
//
// Bounded work.  A query that has visited more than `cell_budget` cells without closing drops its list and scans all M targets (a query far
// outside the targets' box does this: its own cell is clamped into the grid and the faces between it and the far side all count).  Every
// loop is bounded by the grid or by M, no workgroup waits on another, and no address depends on a coordinate other than through the
// clamped cell index; the sort permutations and the cell table are clamped into range where they are read.
#include "dn_common.h"
#include "../../include/diffnet_hip.h"

#define KNG_THREADS 256            /* queries per workgroup: four waves; the lists of k = 32 take 64 KiB of LDS */
#define KNG_CELL_BUDGET 512        /* cells a query may visit before it scans instead */

namespace {
__device__ __forceinline__ float kng_inf() { return __uint_as_float(0x7f800000u); }

struct KngGrid {
    float lo[3];
    float e, inv, h;
};

template <int D>
__device__ __forceinline__ KngGrid kng_grid(const float* DN_RESTRICT box, int G) {
    KngGrid g;
    float e = 0.f;
#pragma unroll
    for (int d = 0; d < 3; ++d) g.lo[d] = d < D ? box[d] : 0.f;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const float ext = box[D + d] - box[d];
        e = ext > e ? ext : e;                     // (a NaN extent is skipped)
    }
    const bool ok = e > 1e-30f && e < kng_inf();
    g.e = ok ? e : 0.f;
    g.inv = ok ? (float)G / e : 0.f;
    g.h = ok ? e / (float)G : 0.f;
    return g;
}

// clamped cell of the offset coordinate xa = fl(x - lo): NaN and -inf -> 0, +inf -> G - 1
__device__ __forceinline__ int kng_cell(float xa, float inv, int G) {
    const float u = xa * inv;
    return u >= 0.f ? (u < (float)G ? (int)u : G - 1) : 0;
}

// cell keys of the targets (threads 0 .. M-1) and, where skey is given, of the sources (threads M .. M+N-1): key = (c_z G + c_y) G + c_x
template <int D>
__global__ __launch_bounds__(256) void knn_grid_keys_kernel(const float* DN_RESTRICT src, int N, const float* DN_RESTRICT tgt, int M,
                                                            const float* DN_RESTRICT box, int G, int* DN_RESTRICT skey, int* DN_RESTRICT tkey) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)M + (skey ? N : 0);
    if (i >= total) return;
    const KngGrid g = kng_grid<D>(box, G);
    const float* p = i < M ? tgt + i * D : src + (i - M) * D;
    int key = 0;
#pragma unroll
    for (int d = D - 1; d >= 0; --d) key = key * G + kng_cell(p[d] - g.lo[d], g.inv, G);
    if (i < M) tkey[i] = key;
    else skey[i - M] = key;
}

// targets in cell order: ts[j] = (x, y, z, bits of the original index) of target torder[j]; absent coordinates are 0
template <int D>
__global__ __launch_bounds__(256) void knn_grid_gather_kernel(const float* DN_RESTRICT tgt, int M, const long long* DN_RESTRICT torder,
                                                              float4* DN_RESTRICT ts) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    long long p = torder[j];
    p = p < 0 ? 0 : (p >= M ? M - 1 : p);
    const float* t = tgt + p * D;
    ts[j] = make_float4(t[0], D > 1 ? t[1] : 0.f, D > 2 ? t[2] : 0.f, __uint_as_float((unsigned)p));
}

// The sorted k-slot list of lane `t` (slot-major: lane t on bank t) with its k-th entry mirrored in registers.
struct KngList {
    float (*lk)[KNG_THREADS];
    int (*li)[KNG_THREADS];
    int t, k, cnt;
    float wk;      // k-th key once the list is full
    int wi;

    // (key, j) in the total order (key, index); candidates arrive in any order
    __device__ __forceinline__ void insert(float key, int j) {
        if (cnt == k && !(key < wk || (key == wk && j < wi))) return;
        int p = cnt < k ? cnt : k - 1;
        while (p > 0) {
            const float pk = lk[p - 1][t];
            const int pi = li[p - 1][t];
            if (!(pk > key || (pk == key && pi > j))) break;
            lk[p][t] = pk;
            li[p][t] = pi;
            --p;
        }
        lk[p][t] = key;
        li[p][t] = j;
        if (cnt < k) ++cnt;
        if (cnt == k) { wk = lk[k - 1][t]; wi = li[k - 1][t]; }
    }
};

template <int D>
__device__ __forceinline__ void kng_candidate(KngList& L, const float4 p, const float (&q)[3], int self) {
    const int oj = (int)__float_as_uint(p.w);
    if (oj == self) return;
    float df = q[0] - p.x;
    float acc = fmaf(df, df, 0.f);
    if (D > 1) { df = q[1] - p.y; acc = fmaf(df, df, acc); }
    if (D > 2) { df = q[2] - p.z; acc = fmaf(df, df, acc); }
    L.insert(acc, oj);
}

// targets j0 .. j1 - 1 of the sorted array, eight loads in flight at a time (a lane's loop is a chain of dependent latencies otherwise)
template <int D>
__device__ __forceinline__ void kng_scan(KngList& L, const float4* DN_RESTRICT ts, int j0, int j1, const float (&q)[3], int self) {
    int j = j0;
    for (; j + 8 <= j1; j += 8) {
        float4 p[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) p[u] = ts[j + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) kng_candidate<D>(L, p[u], q, self);
    }
    for (; j < j1; ++j) kng_candidate<D>(L, ts[j], q, self);
}

// lane i of the launch owns query sorder[i]; info[0]: the largest shell any query reached, info[1]: the queries that scanned
template <int D>
__global__ __launch_bounds__(KNG_THREADS) void knn_grid_search_kernel(const float* DN_RESTRICT src, int N, const float4* DN_RESTRICT ts, int M,
                                                                      const int* DN_RESTRICT cell_start, const long long* DN_RESTRICT sorder,
                                                                      const float* DN_RESTRICT box, int G, int k, int omit, int budget,
                                                                      float* DN_RESTRICT dist, long long* DN_RESTRICT idx, unsigned* info) {
    DN_DYN_SMEM(smem);
    KngList L;
    L.lk = reinterpret_cast<float (*)[KNG_THREADS]>(smem);
    L.li = reinterpret_cast<int (*)[KNG_THREADS]>(smem + (size_t)k * KNG_THREADS * sizeof(float));
    L.t = threadIdx.x; L.k = k; L.cnt = 0; L.wk = kng_inf(); L.wi = 0;
    const long long q0 = (long long)blockIdx.x * KNG_THREADS;
    const int nq = (int)((long long)N - q0 < KNG_THREADS ? (long long)N - q0 : KNG_THREADS);
    const int Gd[3] = {G, D > 1 ? G : 1, D > 2 ? G : 1};

    if ((int)threadIdx.x < nq) {
        long long row = sorder[q0 + threadIdx.x];
        row = row < 0 ? 0 : (row >= N ? N - 1 : row);
        const int self = omit ? (int)row : -1;
        const KngGrid g = kng_grid<D>(box, G);
        float q[3] = {0.f, 0.f, 0.f}, qa[3] = {0.f, 0.f, 0.f};
        int c[3] = {0, 0, 0};
#pragma unroll
        for (int d = 0; d < D; ++d) {
            q[d] = src[row * D + d];
            qa[d] = q[d] - g.lo[d];
            c[d] = kng_cell(qa[d], g.inv, G);
        }
        int visited = 0, r = 0;
        bool scan = budget == 0;                                   // budget 0: every query scans
        for (; !scan; ++r) {                                           // at most G shells: shell G - 1 covers the grid from any cell
            const int z0 = c[2] - r > 0 ? c[2] - r : 0, z1 = c[2] + r < Gd[2] - 1 ? c[2] + r : Gd[2] - 1;
            const int y0 = c[1] - r > 0 ? c[1] - r : 0, y1 = c[1] + r < Gd[1] - 1 ? c[1] + r : Gd[1] - 1;
            const int x0 = c[0] - r > 0 ? c[0] - r : 0, x1 = c[0] + r < G - 1 ? c[0] + r : G - 1;
            for (int z = z0; z <= z1; ++z)
                for (int y = y0; y <= y1; ++y) {
                    const int base = (z * Gd[1] + y) * G;
                    const int dz = z > c[2] ? z - c[2] : c[2] - z, dy = y > c[1] ? y - c[1] : c[1] - y;
                    if (dz == r || dy == r) {                      // a row of the shell's surface: cells x0 .. x1 are one range of targets
                        int j0 = cell_start[base + x0], j1 = cell_start[base + x1 + 1];
                        j0 = j0 < 0 ? 0 : j0; j1 = j1 > M ? M : j1;
                        kng_scan<D>(L, ts, j0, j1, q, self);
                        visited += x1 - x0 + 1;
                    } else {                                       // an interior row: the two end cells, where they are in the grid
                        if (c[0] - r >= 0) {
                            int j0 = cell_start[base + c[0] - r], j1 = cell_start[base + c[0] - r + 1];
                            j0 = j0 < 0 ? 0 : j0; j1 = j1 > M ? M : j1;
                            kng_scan<D>(L, ts, j0, j1, q, self);
                            ++visited;
                        }
                        if (c[0] + r <= G - 1) {
                            int j0 = cell_start[base + c[0] + r], j1 = cell_start[base + c[0] + r + 1];
                            j0 = j0 < 0 ? 0 : j0; j1 = j1 > M ? M : j1;
                            kng_scan<D>(L, ts, j0, j1, q, self);
                            ++visited;
                        }
                    }
                }
            // the closing rule (derivation at the top of the file)
            bool covered = true;
            float lb = kng_inf();
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const float m = (g.e > fabsf(qa[d]) ? g.e : fabsf(qa[d])) * 9.5367431640625e-07f;   // 2^-20 max(e, |qa|)
                if (c[d] - r > 0) {
                    covered = false;
                    const float fp = (float)(c[d] - r) * g.h;
                    const float b = (qa[d] - fp) - m;
                    lb = b < lb ? b : (b == b ? lb : 0.f);         // (a NaN bound never closes)
                }
                if (c[d] + r < G - 1) {
                    covered = false;
                    const float fp = (float)(c[d] + r + 1) * g.h;
                    const float b = (fp - qa[d]) - m;
                    lb = b < lb ? b : (b == b ? lb : 0.f);
                }
            }
            if (covered) break;                                    // every cell has been seen
            if (L.cnt == k && lb > 1e-18f && L.wk < (lb * lb) * 0.99999904632568359375f) break;   // (1 - 2^-20)
            if (visited > budget) { scan = true; break; }
        }
        if (scan) {
            L.cnt = 0;
            kng_scan<D>(L, ts, 0, M, q, self);
        }
        if (info) {
            if ((unsigned)r > *reinterpret_cast<volatile unsigned*>(&info[0])) atomicMax(&info[0], (unsigned)r);
            if (scan) atomicAdd(&info[1], 1u);
        }
    }
    __syncthreads();
    // the finished lists -> rows sorder[q0 + q]: k consecutive words per row
    const int total = nq * k;
    for (int i = threadIdx.x; i < total; i += KNG_THREADS) {
        const int ql = i / k, e = i - ql * k;
        long long row = sorder[q0 + ql];
        row = row < 0 ? 0 : (row >= N ? N - 1 : row);
        dist[row * k + e] = sqrtf(L.lk[e][ql]);
        idx[row * k + e] = (long long)L.li[e][ql];
    }
}

inline int kng_cap(int dim) { return dim == 3 ? 256 : (dim == 2 ? 4096 : (1 << 22)); }   /* at most 2^24 cells */

// G of a call: a host function of (M, k, D).  The library's choice is sized for a cloud that FILLS its box: M / G^D = k / 4 targets per
// cell in 3-D (a ball of radius one cell edge then holds about k of them and the 27 cells of shell 1 about 7 k), k / 2 in 2-D, k in 1-D, so
// the search closes after shell 1 or 2.  A surface in 3-D occupies far fewer cells and meets more candidates per cell than it needs; that
// costs distance evaluations, which are cheap and grow linearly.  The opposite mistake -- a grid sized for a surface under a volume-filling
// cloud -- costs empty cells that grow with the cube of the shell radius and ends in the scan.  A forced value is clamped to the same cap.
inline int knn_grid_resolve(int n_tgt, int k, int dim, int cells_per_axis) {
    const int cap = kng_cap(dim);
    if (cells_per_axis > 0) return cells_per_axis < cap ? cells_per_axis : cap;
    const double per = (double)(n_tgt > 0 ? n_tgt : 1) / (double)(k > 0 ? k : 1);
    double g = dim == 3 ? cbrt(4.0 * per) : (dim == 2 ? sqrt(2.0 * per) : per);
    g = ceil(g);
    return g < 1.0 ? 1 : (g > (double)cap ? cap : (int)g);
}
inline long long kng_n_cells(int G, int dim) { return dim == 3 ? (long long)G * G * G : (dim == 2 ? (long long)G * G : (long long)G); }
inline bool kng_bad_shape(int n_src, int n_tgt, int dim, int k, int omit_diagonal, int cells_per_axis) {
    if (n_src < 0 || n_tgt < 0 || cells_per_axis < 0 || dim < 1 || dim > 3 || k < 1 || k > DN_KNN_MAX_K) return true;
    if (omit_diagonal && n_src != n_tgt) return true;
    return (long long)k > (long long)n_tgt - (omit_diagonal ? 1 : 0);
}
}  // namespace

extern "C" {

int dn_knn_grid_cells(int n_tgt, int k, int dim, int cells_per_axis) {
    if (dim < 1 || dim > 3 || cells_per_axis < 0) return 0;
    return knn_grid_resolve(n_tgt, k, dim, cells_per_axis);
}

int dn_knn_grid_cell_budget(void) { return KNG_CELL_BUDGET; }

size_t dn_knn_grid_workspace_bytes(int n_src, int n_tgt, int dim, int k, int cells_per_axis) {
    (void)cells_per_axis;
    if (n_src <= 0 || n_tgt <= 0 || k < 1 || dim < 1 || dim > 3) return 0;
    return (size_t)n_tgt * sizeof(float4) + 512;
}

int dn_knn_grid_keys_f32(const float* src, int n_src, const float* tgt, int n_tgt, int dim, int k, int cells_per_axis, const float* box,
                         int32_t* src_key, int32_t* tgt_key, void* stream) {
    if (n_src < 0 || n_tgt < 0 || cells_per_axis < 0 || dim < 1 || dim > 3 || k < 1 || k > DN_KNN_MAX_K) return 1;   /* hipErrorInvalidValue */
    if (n_tgt == 0) return 0;
    if (!tgt || !box || !tgt_key || (src_key && n_src > 0 && !src)) return 1;
    const int G = knn_grid_resolve(n_tgt, k, dim, cells_per_axis);
    const long long total = (long long)n_tgt + (src_key ? n_src : 0);
    const dim3 grid((unsigned)((total + 255) / 256), 1, 1);
    hipStream_t st = (hipStream_t)stream;
    if (dim == 1) DN_LAUNCH(knn_grid_keys_kernel<1>, grid, dim3(256, 1, 1), 0, st, src, n_src, tgt, n_tgt, box, G, (int*)src_key, (int*)tgt_key);
    else if (dim == 2) DN_LAUNCH(knn_grid_keys_kernel<2>, grid, dim3(256, 1, 1), 0, st, src, n_src, tgt, n_tgt, box, G, (int*)src_key, (int*)tgt_key);
    else DN_LAUNCH(knn_grid_keys_kernel<3>, grid, dim3(256, 1, 1), 0, st, src, n_src, tgt, n_tgt, box, G, (int*)src_key, (int*)tgt_key);
    return (int)hipGetLastError();
}

int dn_knn_grid_search_f32(const float* src, int n_src, const float* tgt, int n_tgt, int dim, int k, int omit_diagonal, int cells_per_axis,
                           int cell_budget, const float* box, const int64_t* src_order, const int64_t* tgt_order, const int32_t* cell_start,
                           float* dist, int64_t* idx, int32_t* info, void* ws, size_t ws_bytes, void* stream) {
    if (kng_bad_shape(n_src, n_tgt, dim, k, omit_diagonal, cells_per_axis)) return 1;   /* hipErrorInvalidValue */
    if (n_src == 0) return 0;
    if (!src || !tgt || !box || !src_order || !tgt_order || !cell_start || !dist || !idx) return 1;
    if (!ws || ws_bytes < dn_knn_grid_workspace_bytes(n_src, n_tgt, dim, k, cells_per_axis)) return 1;
    const int G = knn_grid_resolve(n_tgt, k, dim, cells_per_axis);
    const int budget = cell_budget < 0 ? KNG_CELL_BUDGET : cell_budget;
    const size_t mis = (256 - ((uintptr_t)ws & 255)) & 255;
    float4* ts = (float4*)((char*)ws + mis);
    hipStream_t st = (hipStream_t)stream;
    const dim3 tgrid((unsigned)(((long long)n_tgt + 255) / 256), 1, 1);
    const dim3 qgrid((unsigned)(((long long)n_src + KNG_THREADS - 1) / KNG_THREADS), 1, 1);
    const size_t smem = (size_t)k * KNG_THREADS * (sizeof(float) + sizeof(int));        /* <= 64 KiB at k = 32 */
    dn_prof_begin(DN_K_SMALL, st);
#define KNG_GO(D_)                                                                                                                          \
    do {                                                                                                                                    \
        DN_LAUNCH(knn_grid_gather_kernel<D_>, tgrid, dim3(256, 1, 1), 0, st, tgt, n_tgt, (const long long*)tgt_order, ts);                  \
        DN_LAUNCH(knn_grid_search_kernel<D_>, qgrid, dim3(KNG_THREADS, 1, 1), smem, st, src, n_src, (const float4*)ts, n_tgt,               \
                  (const int*)cell_start, (const long long*)src_order, box, G, k, omit_diagonal != 0, budget, dist, (long long*)idx,        \
                  (unsigned*)info);                                                                                                         \
    } while (0)
    if (dim == 1) KNG_GO(1);
    else if (dim == 2) KNG_GO(2);
    else KNG_GO(3);
#undef KNG_GO
    dn_prof_end(DN_K_SMALL, st, 0.0, 4.0 * ((double)n_src * dim + 4.0 * n_tgt + 3.0 * (double)n_src * k));
    return (int)hipGetLastError();
}

}  // extern "C"
