// dn_cloud_lap.hip -- Laplacian and lumped mass of a point cloud from local Delaunay stars: the construction of Sharp & Crane, "A Laplacian
// for Nonmanifold Triangle Meshes" (2020), section 5.7, WITHOUT its intrinsic / tufted re-triangulation of the resulting triangle soup.
//
// Three kernels, with a stable device sort of 64-bit keys between the second and the third (the caller's: torch.sort is plumbing):
//   star   per point i, the neighbours projected on the tangent plane (frame rows basisX, basisY) and the star of the origin in their planar
//          Delaunay triangulation.  The lane-group map of dn_cloud.hip: 32 lanes (= DN_KNN_MAX_K) own a point, lane a its neighbour a, a
//          256-thread workgroup 8 points; (X, Y, W = X^2 + Y^2) of the group go to LDS as one 32-byte record per slot (two wide reads, the
//          same address for the 32 lanes of a group: a broadcast, no bank conflict).  Lane a looks for its counter-clockwise partner b: it
//          pivots over the slots c with cross(a, c) > 0 -- the predicate "c is strictly inside circle(0, a, b)" orders the points of one side
//          of the line (0, a) totally, so one pass ends at the only candidate whose circle holds no point of that side -- and then checks
//          that circle against every slot.  About 2 k in-circle tests per lane; a triangle is found once, by the lane on its clockwise side.
//          Ties (co-circular points, in-circle == 0) are "not inside": the pivot keeps the lower slot, the check passes.
//   emit   per filled slot, the cotangent weights and the area of the 3-D triangle (i, nbr[i,a], nbr[i,b]): nine (row, col, value) triples
//          for L and three (vertex, value) for the mass at fixed offsets of the slot, empty slots a key that sorts last.
//   sum    one thread per run of equal sorted keys adds the run in sorted order in fp64 and rounds to fp32 once.
// No floating-point atomic anywhere: the order of every sum is the (stable) sorted one, so the result repeats bit for bit, and entries
// (i, j) and (j, i) are sums of the same terms (each triangle writes the same -w under both keys) in the same order (that of the slots).
// Everything from the coordinate differences on is fp64 (the difference of two fp32 numbers is exact in fp64).
#include "dn_common.h"
#include "../../include/diffnet_hip.h"

#define LP_GROUP DN_KNN_MAX_K   /* lanes per point */
#define LP_PPB 8                /* points per workgroup */
#define LP_CR_TOL 1e-12         /* |cross(a, b)| <= LP_CR_TOL sqrt(W_a W_b): a, b and the centre are collinear -- no triangle */
#define LP_EMPTY 0x7fffffffffffffffLL   /* key of an empty slot: sorts behind every (row << 32 | col) and every vertex */

namespace {
// > 0: c outside circle(0, a, b), < 0: strictly inside, for (a, b) counter-clockwise (cr_ab = cross(a, b) > 0)
__device__ __forceinline__ double lp_incircle(double xa, double ya, double wa, double xb, double yb, double wb, double cr_ab, double xc, double yc,
                                              double wc) {
    return wc * cr_ab - wb * (xa * yc - ya * xc) + wa * (xb * yc - yb * xc);
}

__global__ __launch_bounds__(256) void cloud_star_kernel(const float* DN_RESTRICT pts, int n, const long long* DN_RESTRICT nbr, int k,
                                                         const float* DN_RESTRICT frames, int* partner, int* status) {
    __shared__ double s_p[LP_PPB][LP_GROUP][4];    // X, Y, W, (pad); W == 0: the slot takes no part
    __shared__ int s_bad[LP_PPB][LP_GROUP];

    const int g = threadIdx.x / LP_GROUP, l = threadIdx.x % LP_GROUP;
    const long long i = (long long)blockIdx.x * LP_PPB + g;
    const bool live = i < n;                 // no early return: every thread meets the barrier
    const bool mine = live && l < k;

    long long j = i;
    bool bad = false;
    if (mine) {
        j = nbr[i * k + l];
        bad = j < 0 || j >= n;
        if (bad) j = i;                      // nothing is read through a bad index
    }
    double xa = 0.0, ya = 0.0, wa = 0.0;     // a neighbour equal to i, or one projected onto i: W = 0
    if (mine && j != i) {
        const double ex = (double)pts[3 * j] - (double)pts[3 * i];
        const double ey = (double)pts[3 * j + 1] - (double)pts[3 * i + 1];
        const double ez = (double)pts[3 * j + 2] - (double)pts[3 * i + 2];
        const float* f = frames + 9 * i;
        xa = ex * (double)f[0] + ey * (double)f[1] + ez * (double)f[2];
        ya = ex * (double)f[3] + ey * (double)f[4] + ez * (double)f[5];
        wa = xa * xa + ya * ya;
        if (!(wa > 0.0)) { xa = 0.0; ya = 0.0; wa = 0.0; }     // (NaN coordinates as well: the slot takes no part)
    }
    s_p[g][l][0] = xa; s_p[g][l][1] = ya; s_p[g][l][2] = wa; s_p[g][l][3] = 0.0;
    s_bad[g][l] = bad ? 1 : 0;
    __syncthreads();
    if (!mine) return;                                                    // (the last barrier is behind us)

    int row_bad = 0;
    for (int e = 0; e < k; ++e) row_bad |= s_bad[g][e];
    int b = -1;
    if (!row_bad && wa > 0.0) {
        double xb = 0.0, yb = 0.0, wb = 0.0, cr_ab = 0.0;
        for (int c = 0; c < k; ++c) {
            const double xc = s_p[g][c][0], yc = s_p[g][c][1], wc = s_p[g][c][2];
            if (c == l || !(wc > 0.0)) continue;
            const double cr_ac = xa * yc - ya * xc;
            if (!(cr_ac > LP_CR_TOL * sqrt(wa * wc))) continue;           // not on the counter-clockwise side
            if (b < 0 || lp_incircle(xa, ya, wa, xb, yb, wb, cr_ab, xc, yc, wc) < 0.0) { b = c; xb = xc; yb = yc; wb = wc; cr_ab = cr_ac; }
        }
        if (b >= 0) {
            bool empty = true;
            for (int c = 0; c < k; ++c) {
                const double xc = s_p[g][c][0], yc = s_p[g][c][1], wc = s_p[g][c][2];
                if (c == l || c == b || !(wc > 0.0)) continue;
                if (lp_incircle(xa, ya, wa, xb, yb, wb, cr_ab, xc, yc, wc) < 0.0) empty = false;
            }
            if (!empty) b = -1;
        }
    }
    if (row_bad && l == 0) atomicAdd(status, 1);                          // a row with an index outside [0, n): no triangle, and one count
    partner[i * k + l] = b;
}

// One thread per slot s = i k + a.  L triples at 9 s .. 9 s + 8: the three diagonals (vertices i, j1, j2), then (i,j1) (j1,i) (i,j2) (j2,i)
// (j1,j2) (j2,j1); mass at 3 s .. 3 s + 2 (i, j1, j2).
__global__ __launch_bounds__(256) void cloud_lap_emit_kernel(const float* DN_RESTRICT pts, int n, const long long* DN_RESTRICT nbr, int k,
                                                             const int* DN_RESTRICT partner, long long* key_l, double* val_l, long long* key_m,
                                                             double* val_m) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= (long long)n * k) return;
    const long long i = s / k;
    const int b = partner[s];
    bool filled = b >= 0 && b < k;                                        // nothing is read through a partner or an index out of range
    long long j1 = i, j2 = i;
    if (filled) {
        j1 = nbr[s];
        j2 = nbr[i * k + b];
        filled = j1 >= 0 && j1 < n && j2 >= 0 && j2 < n && j1 != i && j2 != i && j1 != j2;
    }
    double w12 = 0.0, w02 = 0.0, w01 = 0.0, m = 0.0;
    if (filled) {
        const double p0[3] = {(double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2]};
        const double u[3] = {(double)pts[3 * j1] - p0[0], (double)pts[3 * j1 + 1] - p0[1], (double)pts[3 * j1 + 2] - p0[2]};
        const double v[3] = {(double)pts[3 * j2] - p0[0], (double)pts[3 * j2 + 1] - p0[1], (double)pts[3 * j2 + 2] - p0[2]};
        const double t[3] = {v[0] - u[0], v[1] - u[1], v[2] - u[2]};
        const double cx = u[1] * v[2] - u[2] * v[1], cy = u[2] * v[0] - u[0] * v[2], cz = u[0] * v[1] - u[1] * v[0];
        const double cn = sqrt(cx * cx + cy * cy + cz * cz);              // twice the area
        const double d0 = u[0] * v[0] + u[1] * v[1] + u[2] * v[2];        // corner i:  (j1 - i).(j2 - i)
        const double d1 = -(u[0] * t[0] + u[1] * t[1] + u[2] * t[2]);     // corner j1: (i - j1).(j2 - j1)
        const double d2 = v[0] * t[0] + v[1] * t[1] + v[2] * t[2];        // corner j2: (i - j2).(j1 - j2)
        w12 = d0 / cn / 6.0;                                              // cot / 2 of the opposite corner, a third of it
        w02 = d1 / cn / 6.0;
        w01 = d2 / cn / 6.0;
        m = cn / 18.0;                                                    // area / 3, a third of it
        filled = cn > 0.0 && w12 - w12 == 0.0 && w02 - w02 == 0.0 && w01 - w01 == 0.0;   // a degenerate lifted triangle emits nothing
    }
    long long* kl = key_l + 9 * s;
    double* vl = val_l + 9 * s;
    long long* km = key_m + 3 * s;
    double* vm = val_m + 3 * s;
    if (!filled) {
#pragma unroll
        for (int q = 0; q < 9; ++q) { kl[q] = LP_EMPTY; vl[q] = 0.0; }
#pragma unroll
        for (int q = 0; q < 3; ++q) { km[q] = LP_EMPTY; vm[q] = 0.0; }
        return;
    }
    const long long r0 = i << 32, r1 = j1 << 32, r2 = j2 << 32;
    kl[0] = r0 | i;  vl[0] = w01 + w02;
    kl[1] = r1 | j1; vl[1] = w01 + w12;
    kl[2] = r2 | j2; vl[2] = w02 + w12;
    kl[3] = r0 | j1; vl[3] = -w01;
    kl[4] = r1 | i;  vl[4] = -w01;
    kl[5] = r0 | j2; vl[5] = -w02;
    kl[6] = r2 | i;  vl[6] = -w02;
    kl[7] = r1 | j2; vl[7] = -w12;
    kl[8] = r2 | j1; vl[8] = -w12;
    km[0] = i;  vm[0] = m;
    km[1] = j1; vm[1] = m;
    km[2] = j2; vm[2] = m;
}

// One thread per position p of the sorted keys; the thread at the head of a run of equal keys owns it.  rowptr != NULL: keys are
// (row << 32 | col), the run of rank r (rank[p] - 1, the caller's inclusive count of run heads) goes to col[r] / out[r], and the thread
// fills the row pointers between the row of the run before it and its own (the last run: up to n_rows).  rowptr == NULL: keys are indices
// into out [n_rows], which the caller has zeroed.
__global__ __launch_bounds__(256) void segment_sum_kernel(const long long* DN_RESTRICT keys, const long long* DN_RESTRICT perm,
                                                          const double* DN_RESTRICT vals, int m, const long long* DN_RESTRICT rank, int n_rows,
                                                          int* rowptr, int* col, float* out, int* count) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const long long key = keys[p];
    const long long before = p > 0 ? keys[p - 1] : -1;
    if (key == before && p > 0) return;                                   // not the head of a run
    const long long row = rowptr ? (key >> 32) : key;
    const long long c = key & 0xffffffffLL;
    const bool valid = key != LP_EMPTY && row >= 0 && row < n_rows && (!rowptr || c < n_rows);
    if (rowptr) {
        const long long r = rank[p] - 1;                                  // runs before this one
        long long row_before = p > 0 ? (before >> 32) : -1;
        if (row_before >= n_rows) row_before = n_rows - 1;
        if (row_before < -1) row_before = -1;
        if (!valid) {                                                     // the first key that is no entry: the rows behind the last run
            if (r >= 0 && r <= m) {
                for (long long rr = row_before + 1; rr <= n_rows; ++rr) rowptr[rr] = (int)r;
                *count = (int)r;
            }
            return;
        }
        if (r < 0 || r >= m) return;
        for (long long rr = row_before + 1; rr <= row; ++rr) rowptr[rr] = (int)r;
        double sum = 0.0;
        long long q = p;
        for (; q < m && keys[q] == key; ++q) {
            const long long src = perm[q];
            if (src >= 0 && src < m) sum += vals[src];
        }
        col[r] = (int)c;
        out[r] = (float)sum;
        if (q == m) {                                                     // the last run reaches the end of the keys
            for (long long rr = row + 1; rr <= n_rows; ++rr) rowptr[rr] = (int)(r + 1);
            *count = (int)(r + 1);
        }
        return;
    }
    if (!valid) return;
    double sum = 0.0;
    for (long long q = p; q < m && keys[q] == key; ++q) {
        const long long src = perm[q];
        if (src >= 0 && src < m) sum += vals[src];
    }
    out[row] = (float)sum;
}

inline bool lp_bad_shape(int n, int k) { return k < 1 || k > DN_KNN_MAX_K || n < 0 || 9LL * n * k > 2147483647LL; }
}  // namespace

extern "C" {

size_t dn_cloud_laplacian_workspace_bytes(int n, int k) {
    if (lp_bad_shape(n, k)) return 0;
    return (size_t)192 * (size_t)n * (size_t)k;                           // keys and values: 9 + 9 + 3 + 3 words of 8 bytes per slot
}

int dn_cloud_star_f32(const float* pts, int n, const int64_t* nbr, int k, const float* frames, int32_t* partner, int32_t* status, void* stream) {
    if (lp_bad_shape(n, k)) return 1;   /* hipErrorInvalidValue */
    if (n == 0) return 0;
    if (!pts || !nbr || !frames || !partner || !status) return 1;
    hipStream_t st = (hipStream_t)stream;
    (void)hipMemsetAsync(status, 0, sizeof(int32_t), st);
    const unsigned nb = (unsigned)(((long long)n + LP_PPB - 1) / LP_PPB);
    const double rows = (double)n, kk = (double)k;
    dn_prof_begin(DN_K_SMALL, st);
    DN_LAUNCH(cloud_star_kernel, dim3(nb, 1, 1), dim3(LP_GROUP * LP_PPB, 1, 1), 0, st, pts, n, (const long long*)nbr, k, frames, (int*)partner,
              (int*)status);
    dn_prof_end(DN_K_SMALL, st, rows * kk * (2.0 * kk * 14.0 + 20.0), rows * (8.0 * kk + 12.0 * kk + 12.0 + 36.0 + 4.0 * kk));
    return (int)hipGetLastError();
}

int dn_cloud_laplacian_emit_f32(const float* pts, int n, const int64_t* nbr, int k, const int32_t* partner, void* ws, size_t ws_bytes, void* stream) {
    if (lp_bad_shape(n, k)) return 1;
    if (n == 0) return 0;
    if (!pts || !nbr || !partner || !ws) return 1;
    if (ws_bytes < dn_cloud_laplacian_workspace_bytes(n, k)) return 1;
    hipStream_t st = (hipStream_t)stream;
    const long long slots = (long long)n * k;
    long long* key_l = (long long*)ws;
    double* val_l = (double*)(key_l + 9 * slots);
    long long* key_m = (long long*)(val_l + 9 * slots);
    double* val_m = (double*)(key_m + 3 * slots);
    const unsigned nb = (unsigned)((slots + 255) / 256);
    dn_prof_begin(DN_K_SMALL, st);
    DN_LAUNCH(cloud_lap_emit_kernel, dim3(nb, 1, 1), dim3(256, 1, 1), 0, st, pts, n, (const long long*)nbr, k, (const int*)partner, key_l, val_l,
              key_m, val_m);
    dn_prof_end(DN_K_SMALL, st, (double)slots * 60.0, (double)slots * (4.0 + 16.0 + 36.0 + 192.0));
    return (int)hipGetLastError();
}

int dn_segment_sum_f64_f32(const int64_t* keys, const int64_t* perm, const double* vals, int m, const int64_t* rank, int n_rows, int32_t* rowptr,
                           int32_t* col, float* out, int32_t* count, void* stream) {
    if (m < 0 || n_rows < 0) return 1;   /* hipErrorInvalidValue */
    if (m == 0 && n_rows == 0) return 0;
    const bool csr = rowptr != nullptr;
    if (!out || (csr && (!col || !count))) return 1;
    if (m > 0 && (!keys || !perm || !vals || (csr && !rank))) return 1;
    hipStream_t st = (hipStream_t)stream;
    if (csr) {                                                            // (no key at all: every row is empty)
        (void)hipMemsetAsync(rowptr, 0, sizeof(int32_t) * ((size_t)n_rows + 1), st);
        (void)hipMemsetAsync(count, 0, sizeof(int32_t), st);
    } else if (n_rows > 0) {
        (void)hipMemsetAsync(out, 0, sizeof(float) * (size_t)n_rows, st);
    }
    if (m == 0) return (int)hipGetLastError();
    const unsigned nb = (unsigned)(((long long)m + 255) / 256);
    dn_prof_begin(DN_K_SMALL, st);
    DN_LAUNCH(segment_sum_kernel, dim3(nb, 1, 1), dim3(256, 1, 1), 0, st, (const long long*)keys, (const long long*)perm, vals, m,
              (const long long*)rank, n_rows, (int*)rowptr, (int*)col, out, (int*)count);
    dn_prof_end(DN_K_SMALL, st, (double)m, (double)m * 32.0);
    return (int)hipGetLastError();
}

}  // extern "C"
