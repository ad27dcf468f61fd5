// dn_cloud.hip -- the per-point part of the reference's point-cloud precompute in one pass over a neighbour table: normal
// (vertex_normals + neighborhood_normal, geometry.py:92-99, 114-123), tangent frame (build_tangent_frames, :151-177) and the least-squares
// gradient stencil (edge_tangent_vectors + build_grad over the (i, nbr[i, j]) edge list, :179-273).
//
// Mapping: a group of 32 lanes (= DN_KNN_MAX_K) owns one point, lane j its neighbour j; a 256-thread workgroup owns 8 points.  The k scattered
// 12-byte gathers of a point are then ONE wave instruction (two points per wave) instead of k dependent trips of one thread, and the k + 1
// entries of a gradient row leave as one contiguous store per array.  What the lanes of a point share -- the six sums of P^T P, the three of
// G, the two of the self coefficient -- goes through LDS: every lane writes its term, and after a barrier every lane adds the k terms in the
// order j = 0 .. k-1.  All lanes of a group therefore hold the same bits, the order of every sum is fixed (deterministic from run to run),
// and no cross-lane instruction is needed (the same source runs on the fiber emulator).  The 3 x 3 eigenproblem and the 2 x 2 inverse are
// solved redundantly by the 32 lanes: a wave pays for them once per two points.  Measured (profiles/cloud_timing.txt): 0.47 ms for 200 000
// points, 0.44 TB/s of bytes moved -- bound by this redundant fp64 work and the LDS sums, not by the gathers, and 1 % of the neighbour query.
//
// Arithmetic: the coordinate differences of two fp32 numbers are exact in fp64, and everything after them is fp64; results are rounded to
// fp32 once, at the store.  The smallest eigenvector of P^T P comes from CL_SWEEPS cyclic Jacobi sweeps (rotations (0,1), (0,2), (1,2)):
// the accumulated rotations are orthonormal whatever the matrix, so rank-deficient neighbourhoods (collinear or coincident points) still
// give a finite unit vector -- one orthogonal to the line for collinear ones.
#include "dn_common.h"
#include "../../include/diffnet_hip.h"

#define CL_GROUP DN_KNN_MAX_K   /* lanes per point */
#define CL_PPB 8                /* points per workgroup */
#define CL_SWEEPS 8             /* cyclic Jacobi converges quadratically: a 3 x 3 matrix is at fp64 round-off after 4-5 sweeps */
#define CL_GRAD_REG 1e-5        /* geometry.py:233 */
#define CL_NORM_EPS 1e-6        /* normalize(), geometry.py:38-48 */

namespace {
// One Jacobi rotation in the (p, q) plane of a symmetric 3 x 3 matrix (r: the third index); vp / vq: columns p and q of the accumulated rotations.
__device__ __forceinline__ void cl_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double* vp, double* vq) {
    double c = 1.0, s = 0.0, t = 0.0;
    if (apq != 0.0) {
        const double theta = (aqq - app) / (2.0 * apq);
        t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));   // |theta| huge: t -> 0, never NaN
        c = 1.0 / sqrt(t * t + 1.0);
        s = t * c;
    }
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double a = vp[d], b = vq[d];
        vp[d] = c * a - s * b;
        vq[d] = s * a + c * b;
    }
}

// Unit eigenvector of the smallest eigenvalue of the symmetric matrix [a00 a01 a02; . a11 a12; . . a22]; equal eigenvalues: the lower column.
__device__ __forceinline__ void cl_smallest_eigvec(double a00, double a01, double a02, double a11, double a12, double a22, double* nrm) {
    double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};
#pragma unroll 1
    for (int sweep = 0; sweep < CL_SWEEPS; ++sweep) {
        cl_rotate(a00, a11, a01, a02, a12, v0, v1);
        cl_rotate(a00, a22, a02, a01, a12, v0, v2);
        cl_rotate(a11, a22, a12, a01, a02, v1, v2);
    }
    double x = v0[0], y = v0[1], z = v0[2], lo = a00;
    if (a11 < lo) { x = v1[0]; y = v1[1]; z = v1[2]; lo = a11; }
    if (a22 < lo) { x = v2[0]; y = v2[1]; z = v2[2]; }
    const double inv = 1.0 / sqrt(x * x + y * y + z * z);                 // the columns are unit up to round-off: never zero
    nrm[0] = x * inv; nrm[1] = y * inv; nrm[2] = z * inv;
}

// v[d] for a lane-dependent d without a runtime-indexed register array
__device__ __forceinline__ double cl_pick(const double* v, int d) { return d == 0 ? v[0] : d == 1 ? v[1] : v[2]; }

// what a call reads and writes: k indices and k gathered points, its own point, normal, frame, row pointer and the k + 1 row entries
inline double cloud_bytes_moved(int n, int k) { return (double)n * (8.0 * k + 12.0 * k + 12.0 + 12.0 + 36.0 + 4.0 + 12.0 * (k + 1)); }

__global__ __launch_bounds__(256) void cloud_kernel(const float* DN_RESTRICT pts, int n, const long long* DN_RESTRICT nbr, int k,
                                                    const float* normals_in, float* normals, float* frames, int* g_rowptr, int* g_col,
                                                    float* g_vx, float* g_vy, int* status) {
    __shared__ double s_cov[CL_PPB][6][CL_GROUP];
    __shared__ double s_g[CL_PPB][3][CL_GROUP];
    __shared__ double s_c[CL_PPB][2][CL_GROUP];
    __shared__ int s_bad[CL_PPB][CL_GROUP];

    const int g = threadIdx.x / CL_GROUP, l = threadIdx.x % CL_GROUP;
    const long long i = (long long)blockIdx.x * CL_PPB + g;
    const bool live = i < n;                 // no early return: every thread meets every barrier
    const bool mine = live && l < k;

    long long j = i;
    bool bad = false;
    if (mine) {
        j = nbr[i * k + l];
        bad = j < 0 || j >= n;
        if (bad) j = i;                      // nothing is read through a bad index
    }
    double ex = 0.0, ey = 0.0, ez = 0.0;     // a neighbour equal to i is the reference's dropped tail == tip edge: it contributes nothing
    if (mine && j != i) {
        ex = (double)pts[3 * j] - (double)pts[3 * i];
        ey = (double)pts[3 * j + 1] - (double)pts[3 * i + 1];
        ez = (double)pts[3 * j + 2] - (double)pts[3 * i + 2];
    }
    s_bad[g][l] = bad ? 1 : 0;
    if (!normals_in) {
        s_cov[g][0][l] = ex * ex; s_cov[g][1][l] = ex * ey; s_cov[g][2][l] = ex * ez;
        s_cov[g][3][l] = ey * ey; s_cov[g][4][l] = ey * ez; s_cov[g][5][l] = ez * ez;
    }
    __syncthreads();

    int row_bad = 0;
    for (int e = 0; e < k; ++e) row_bad |= s_bad[g][e];
    double nrm[3] = {0.0, 0.0, 1.0};
    if (normals_in) {
        if (live) { nrm[0] = (double)normals_in[3 * i]; nrm[1] = (double)normals_in[3 * i + 1]; nrm[2] = (double)normals_in[3 * i + 2]; }
    } else {
        double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int e = 0; e < k; ++e) {
#pragma unroll
            for (int q = 0; q < 6; ++q) a[q] += s_cov[g][q][e];
        }
        cl_smallest_eigvec(a[0], a[1], a[2], a[3], a[4], a[5], nrm);
        // the sign LAPACK leaves open: the component of largest magnitude is positive, ties to the lower axis
        double lead = nrm[0];
        if (fabs(nrm[1]) > fabs(lead)) lead = nrm[1];
        if (fabs(nrm[2]) > fabs(lead)) lead = nrm[2];
        if (lead < 0.0) { nrm[0] = -nrm[0]; nrm[1] = -nrm[1]; nrm[2] = -nrm[2]; }
    }

    // build_tangent_frames: e_x (e_y where |n_x| >= 0.9) projected on the tangent plane, divided by (norm + 1e-6); by = n x bx
    const bool use_x = fabs(nrm[0]) < 0.9;
    const double cx0 = use_x ? 1.0 : 0.0, cy0 = use_x ? 0.0 : 1.0;
    const double dotc = use_x ? nrm[0] : nrm[1];
    double bx[3] = {cx0 - nrm[0] * dotc, cy0 - nrm[1] * dotc, 0.0 - nrm[2] * dotc};
    const double binv = 1.0 / (sqrt(bx[0] * bx[0] + bx[1] * bx[1] + bx[2] * bx[2]) + CL_NORM_EPS);
    bx[0] *= binv; bx[1] *= binv; bx[2] *= binv;
    const double by[3] = {nrm[1] * bx[2] - nrm[2] * bx[1], nrm[2] * bx[0] - nrm[0] * bx[2], nrm[0] * bx[1] - nrm[1] * bx[0]};

    // edge_tangent_vectors + build_grad: G = sum t t^T + 1e-5 I, coefficient of neighbour j = G^-1 t_j, of i itself = -sum_j G^-1 t_j
    const double tx = ex * bx[0] + ey * bx[1] + ez * bx[2];
    const double ty = ex * by[0] + ey * by[1] + ez * by[2];
    s_g[g][0][l] = tx * tx; s_g[g][1][l] = tx * ty; s_g[g][2][l] = ty * ty;
    __syncthreads();
    double gxx = 0.0, gxy = 0.0, gyy = 0.0;
    for (int e = 0; e < k; ++e) { gxx += s_g[g][0][e]; gxy += s_g[g][1][e]; gyy += s_g[g][2][e]; }
    gxx += CL_GRAD_REG;
    gyy += CL_GRAD_REG;
    const double det = gxx * gyy - gxy * gxy;                             // >= 1e-10: G is positive definite
    const double ixx = gyy / det, ixy = -gxy / det, iyy = gxx / det;
    const double cx = ixx * tx + ixy * ty, cy = ixy * tx + iyy * ty;
    s_c[g][0][l] = cx; s_c[g][1][l] = cy;
    __syncthreads();
    if (!live) return;                                                    // (the last barrier is behind us)

    const long long base = i * (long long)(k + 1);
    if (l == 0) {
        g_rowptr[i] = (int)base;
        if (i == n - 1) g_rowptr[n] = (int)(base + k + 1);
    }
    if (row_bad) {                                                        // a row with an index outside [0, n): zeros, and one count
        if (l == 0) { atomicAdd(status, 1); g_col[base] = 0; g_vx[base] = 0.f; g_vy[base] = 0.f; }
        if (l < 3) normals[3 * i + l] = 0.f;
        if (l < 9) frames[9 * i + l] = 0.f;
        if (l < k) { g_col[base + 1 + l] = 0; g_vx[base + 1 + l] = 0.f; g_vy[base + 1 + l] = 0.f; }
        return;
    }
    if (l == 0) {
        double sx = 0.0, sy = 0.0;
        for (int e = 0; e < k; ++e) { sx += s_c[g][0][e]; sy += s_c[g][1][e]; }
        g_col[base] = (int)i;
        g_vx[base] = (float)(-sx);
        g_vy[base] = (float)(-sy);
    }
    // (normals_in given: nrm holds its fp32 values, which the conversion back returns unchanged -- the copy the header promises)
    if (l < 3) normals[3 * i + l] = (float)cl_pick(nrm, l);
    if (l < 9) {
        const int r = l / 3, d = l - 3 * r;
        frames[9 * i + l] = (float)(r == 0 ? cl_pick(bx, d) : r == 1 ? cl_pick(by, d) : cl_pick(nrm, d));
    }
    if (l < k) {
        g_col[base + 1 + l] = (int)j;
        g_vx[base + 1 + l] = (float)cx;
        g_vy[base + 1 + l] = (float)cy;
    }
}
}  // namespace

extern "C" {

int dn_cloud_operators_f32(const float* pts, int n, const int64_t* nbr, int k, const float* normals_in, float* normals, float* frames,
                           int32_t* g_rowptr, int32_t* g_col, float* g_vx, float* g_vy, int32_t* status, void* stream) {
    if (k < 1 || k > DN_KNN_MAX_K || n < 0) return 1;   /* hipErrorInvalidValue */
    if ((long long)n * (long long)(k + 1) > 2147483647LL) return 1;
    if (n == 0) return 0;
    if (!pts || !nbr || !normals || !frames || !g_rowptr || !g_col || !g_vx || !g_vy || !status) return 1;
    hipStream_t st = (hipStream_t)stream;
    (void)hipMemsetAsync(status, 0, sizeof(int32_t), st);
    const unsigned nb = (unsigned)(((long long)n + CL_PPB - 1) / CL_PPB);
    const double rows = (double)n, kk = (double)k;
    dn_prof_begin(DN_K_SMALL, st);
    DN_LAUNCH(cloud_kernel, dim3(nb, 1, 1), dim3(CL_GROUP * CL_PPB, 1, 1), 0, st, pts, n, (const long long*)nbr, k, normals_in, (float*)normals,
              (float*)frames, (int*)g_rowptr, (int*)g_col, (float*)g_vx, (float*)g_vy, (int*)status);
    dn_prof_end(DN_K_SMALL, st, rows * (40.0 * kk + 600.0), cloud_bytes_moved(n, k));
    return (int)hipGetLastError();
}

}  // extern "C"
