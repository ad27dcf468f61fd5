// dn_mesh.hip -- the operators of a triangle mesh: cotan Laplacian, lumped mass, vertex normal sums, tangent frames and the least-squares
// gradient operator (geometry.py:114-148, 151-177, 209-273, 306-335 for a mesh), the store-and-sum pattern of dn_cloud_lap.hip.
//
// Three kernels, with a stable device sort of 64-bit keys between the first and the second (the caller's: torch.sort is plumbing):
//   emit    one lane per face: the three cotangent weights w = 0.5 (a.b) / (|a x b| + 1e-10), nine (row << 32 | col, value) terms of L,
//           and three (vertex; area / 3, unit face normal) records.  The records of a workgroup's 256 faces are laid out face after face
//           in LDS and leave as one contiguous run of 16-byte stores per array: a lane's own records are 72, 24 and 96 bytes, which no
//           lane-per-face store would coalesce.
//   sum     one thread per run of equal sorted keys adds the run in sorted order in fp64 and stores fp64: L as CSR with ascending columns
//           (one value per key), the vertex records as [V, 4] (four values per key).
//   vertex  one lane per row of L's CSR: the frame of the given normal, then two walks over the row in column order -- G = sum t t^T +
//           1e-5 I, then the coefficients G^-1 t_j into the off-diagonal slots and -sum_j G^-1 t_j into the diagonal slot.
// No floating-point atomic anywhere: the order of every sum is the (stable) sorted one -- face after face, the nine terms of a face in their
// fixed order -- so the result repeats bit for bit, and entries (i, j) and (j, i) are sums of the same terms (each corner writes the same
// -w under both keys, next to each other) in the same order.  Everything from the coordinate differences on is fp64 (the difference of two
// fp32 numbers is exact in fp64).
#include "dn_common.h"
#include "../../include/diffnet_hip.h"

#define MS_FPB 256                      /* faces per workgroup of the face pass */
#define MS_EMPTY 0x7fffffffffffffffLL   /* key of a face that is not emitted: sorts behind every (row << 32 | col) and every vertex */
#define MS_W_EPS 1e-10                  /* cotan_laplacian: denom_eps */
#define MS_N_EPS 1e-6                   /* normalize() of the reference */
#define MS_G_REG 1e-5                   /* gradient_operator: GRAD_REG */

namespace {
struct alignas(16) MsPair { unsigned long long a, b; };

__device__ __forceinline__ unsigned long long ms_bits(double v) { return __builtin_bit_cast(unsigned long long, v); }

// 0.5 (a.b) / (|a x b| + eps) of the corner whose two edges are a and b
__device__ __forceinline__ double ms_half_cot(const double* a, const double* b) {
    const double cx = a[1] * b[2] - a[2] * b[1], cy = a[2] * b[0] - a[0] * b[2], cz = a[0] * b[1] - a[1] * b[0];
    return 0.5 * (a[0] * b[0] + a[1] * b[1] + a[2] * b[2]) / (sqrt(cx * cx + cy * cy + cz * cz) + MS_W_EPS);
}

// the workgroup's `count` 8-byte words of s go to dst (16-byte aligned: the workgroup's first face is a multiple of 256) as 16-byte stores
__device__ __forceinline__ void ms_flush(const unsigned long long* s, unsigned long long* dst, int count) {
    __syncthreads();
    const int pairs = count >> 1;
    for (int p = threadIdx.x; p < pairs; p += MS_FPB) {
        MsPair v;
        v.a = s[2 * p];
        v.b = s[2 * p + 1];
        reinterpret_cast<MsPair*>(dst)[p] = v;
    }
    if ((count & 1) && threadIdx.x == 0) dst[count - 1] = s[count - 1];
    __syncthreads();
}

__global__ __launch_bounds__(MS_FPB) void mesh_emit_kernel(const float* DN_RESTRICT verts, int n_verts, const long long* DN_RESTRICT faces,
                                                           int n_faces, unsigned long long* key_l, unsigned long long* val_l,
                                                           unsigned long long* key_v, unsigned long long* val_v, int* status) {
    __shared__ unsigned long long s_rec[MS_FPB * 12];                     // 24 KiB, one array of records at a time
    const long long f0 = (long long)blockIdx.x * MS_FPB;
    const long long f = f0 + threadIdx.x;
    const int live = (int)((long long)n_faces - f0 < MS_FPB ? (long long)n_faces - f0 : MS_FPB);   // no early return: every thread meets the barriers
    const bool mine = threadIdx.x < live;

    long long v[3] = {0, 0, 0};
    bool ok = false;
    if (mine) {
        v[0] = faces[3 * f]; v[1] = faces[3 * f + 1]; v[2] = faces[3 * f + 2];
        ok = v[0] >= 0 && v[0] < n_verts && v[1] >= 0 && v[1] < n_verts && v[2] >= 0 && v[2] < n_verts;
        if (!ok) atomicAdd(status, 1);                                    // nothing is read through a bad index; one count per face
    }
    double w[3] = {0.0, 0.0, 0.0}, rec[4] = {0.0, 0.0, 0.0, 0.0};
    if (ok) {
        double x[3][3];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int d = 0; d < 3; ++d) x[c][d] = (double)verts[3 * v[c] + d];
#pragma unroll
        for (int c = 0; c < 3; ++c) {                                     // corner c: opposite edge (v[c + 1], v[c + 2])
            const int i = (c + 1) % 3, j = (c + 2) % 3;
            const double a[3] = {x[i][0] - x[c][0], x[i][1] - x[c][1], x[i][2] - x[c][2]};
            const double b[3] = {x[j][0] - x[c][0], x[j][1] - x[c][1], x[j][2] - x[c][2]};
            w[c] = ms_half_cot(a, b);
        }
        const double e1[3] = {x[1][0] - x[0][0], x[1][1] - x[0][1], x[1][2] - x[0][2]};
        const double e2[3] = {x[2][0] - x[0][0], x[2][1] - x[0][1], x[2][2] - x[0][2]};
        const double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
        const double nn = sqrt(nx * nx + ny * ny + nz * nz);              // twice the area
        rec[0] = 0.5 * nn / 3.0;
        rec[1] = nx / (nn + MS_N_EPS);
        rec[2] = ny / (nn + MS_N_EPS);
        rec[3] = nz / (nn + MS_N_EPS);
    }
    const int t = threadIdx.x;
    const unsigned long long r0 = (unsigned long long)v[0] << 32, r1 = (unsigned long long)v[1] << 32, r2 = (unsigned long long)v[2] << 32;
    const unsigned long long c0 = (unsigned long long)v[0], c1 = (unsigned long long)v[1], c2 = (unsigned long long)v[2];

    // keys of L: the diagonals of v0, v1, v2, then (v1,v2) (v2,v1) of corner 0, (v2,v0) (v0,v2) of corner 1, (v0,v1) (v1,v0) of corner 2
    if (mine) {
        unsigned long long* k = s_rec + 9 * t;
        if (ok) {
            k[0] = r0 | c0; k[1] = r1 | c1; k[2] = r2 | c2;
            k[3] = r1 | c2; k[4] = r2 | c1; k[5] = r2 | c0; k[6] = r0 | c2; k[7] = r0 | c1; k[8] = r1 | c0;
        } else {
#pragma unroll
            for (int q = 0; q < 9; ++q) k[q] = (unsigned long long)MS_EMPTY;
        }
    }
    ms_flush(s_rec, key_l + 9 * f0, 9 * live);
    if (mine) {                                                           // (a face that is not emitted: nine zeros)
        unsigned long long* k = s_rec + 9 * t;
        k[0] = ms_bits(w[1] + w[2]); k[1] = ms_bits(w[2] + w[0]); k[2] = ms_bits(w[0] + w[1]);
        k[3] = ms_bits(-w[0]); k[4] = ms_bits(-w[0]); k[5] = ms_bits(-w[1]); k[6] = ms_bits(-w[1]); k[7] = ms_bits(-w[2]); k[8] = ms_bits(-w[2]);
    }
    ms_flush(s_rec, val_l + 9 * f0, 9 * live);
    if (mine) {
        unsigned long long* k = s_rec + 3 * t;
        k[0] = ok ? c0 : (unsigned long long)MS_EMPTY; k[1] = ok ? c1 : (unsigned long long)MS_EMPTY; k[2] = ok ? c2 : (unsigned long long)MS_EMPTY;
    }
    ms_flush(s_rec, key_v + 3 * f0, 3 * live);
    if (mine) {
        unsigned long long* k = s_rec + 12 * t;
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int q = 0; q < 4; ++q) k[4 * c + q] = ms_bits(rec[q]);
    }
    ms_flush(s_rec, val_v + 12 * f0, 12 * live);
}

// One thread per position p of the sorted keys; the thread at the head of a run of equal keys owns it and adds vals[perm[q]] over the run in
// sorted order.  CSR (WIDTH == 1, rowptr != NULL): keys are (row << 32 | col), the run of rank r (rank[p] - 1, the caller's inclusive count
// of run heads) goes to col[r] / out[r], and the thread fills the row pointers between the row of the run before it and its own (the last
// run: up to n_rows).  Dense (rowptr == NULL): keys index the rows of out [n_rows, WIDTH], which the caller has zeroed.
template <int WIDTH>
__global__ __launch_bounds__(256) void mesh_segment_sum_kernel(const long long* DN_RESTRICT keys, const long long* DN_RESTRICT perm,
                                                               const double* DN_RESTRICT vals, int m, const long long* DN_RESTRICT rank, int n_rows,
                                                               int* rowptr, int* col, double* out, int* count) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const long long key = keys[p];
    const long long before = p > 0 ? keys[p - 1] : -1;
    if (key == before && p > 0) return;                                   // not the head of a run
    const long long row = rowptr ? (key >> 32) : key;
    const long long c = key & 0xffffffffLL;
    const bool valid = key != MS_EMPTY && row >= 0 && row < n_rows && (!rowptr || c < n_rows);
    long long r = 0;
    if (rowptr) {
        r = rank[p] - 1;                                                  // runs before this one
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
    } else if (!valid) {
        return;
    }
    double sum[WIDTH];
#pragma unroll
    for (int t = 0; t < WIDTH; ++t) sum[t] = 0.0;
    long long q = p;
    for (; q < m && keys[q] == key; ++q) {
        const long long src = perm[q];
        if (src >= 0 && src < m) {
#pragma unroll
            for (int t = 0; t < WIDTH; ++t) sum[t] += vals[src * WIDTH + t];
        }
    }
    if (rowptr) {
        col[r] = (int)c;
        out[r] = sum[0];
        if (q == m) {                                                     // the last run reaches the end of the keys
            for (long long rr = row + 1; rr <= n_rows; ++rr) rowptr[rr] = (int)(r + 1);
            *count = (int)(r + 1);
        }
        return;
    }
#pragma unroll
    for (int t = 0; t < WIDTH; ++t) out[row * WIDTH + t] = sum[t];
}

// One lane per vertex i = row i of the CSR pattern (rowptr, col).
__global__ __launch_bounds__(256) void mesh_vertex_kernel(const float* DN_RESTRICT verts, int n, const int* DN_RESTRICT rowptr, const int* DN_RESTRICT col,
                                                          int nnz, const double* DN_RESTRICT normals, double* frames, double* gx, double* gy,
                                                          int* status) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double nx = normals[3 * i], ny = normals[3 * i + 1], nz = normals[3 * i + 2];
    const bool use_x = fabs(nx) < 0.9;
    const double cx = use_x ? 1.0 : 0.0, cy = use_x ? 0.0 : 1.0;          // e_x, or e_y where the normal is close to e_x
    const double d = cx * nx + cy * ny;
    double bx0 = cx - nx * d, bx1 = cy - ny * d, bx2 = 0.0 - nz * d;
    const double bn = sqrt(bx0 * bx0 + bx1 * bx1 + bx2 * bx2) + MS_N_EPS;
    bx0 /= bn; bx1 /= bn; bx2 /= bn;
    const double by0 = ny * bx2 - nz * bx1, by1 = nz * bx0 - nx * bx2, by2 = nx * bx1 - ny * bx0;
    double* fr = frames + 9 * i;
    fr[0] = bx0; fr[1] = bx1; fr[2] = bx2; fr[3] = by0; fr[4] = by1; fr[5] = by2; fr[6] = nx; fr[7] = ny; fr[8] = nz;

    const long long e0 = rowptr[i], e1 = rowptr[i + 1];
    if (e0 < 0 || e1 > nnz || e0 > e1) { atomicAdd(status, 1); return; }  // no row to walk: nothing is read or written through it
    const double px = (double)verts[3 * i], py = (double)verts[3 * i + 1], pz = (double)verts[3 * i + 2];
    double gxx = 0.0, gxy = 0.0, gyy = 0.0;
    bool bad = false;
    long long diag = -1;
    for (long long e = e0; e < e1; ++e) {
        const long long j = col[e];
        if (j < 0 || j >= n) { bad = true; continue; }
        if (j == i) { diag = e; continue; }
        const double ex = (double)verts[3 * j] - px, ey = (double)verts[3 * j + 1] - py, ez = (double)verts[3 * j + 2] - pz;
        const double tx = ex * bx0 + ey * bx1 + ez * bx2, ty = ex * by0 + ey * by1 + ez * by2;
        gxx += tx * tx; gxy += tx * ty; gyy += ty * ty;
    }
    gxx += MS_G_REG; gyy += MS_G_REG;
    const double det = gxx * gyy - gxy * gxy;
    const double ixx = gyy / det, ixy = -gxy / det, iyy = gxx / det;
    double sx = 0.0, sy = 0.0;
    for (long long e = e0; e < e1; ++e) {
        const long long j = col[e];
        if (j == i) continue;
        if (j < 0 || j >= n) { gx[e] = 0.0; gy[e] = 0.0; continue; }
        const double ex = (double)verts[3 * j] - px, ey = (double)verts[3 * j + 1] - py, ez = (double)verts[3 * j + 2] - pz;
        const double tx = ex * bx0 + ey * bx1 + ez * bx2, ty = ex * by0 + ey * by1 + ez * by2;
        const double vx = ixx * tx + ixy * ty, vy = ixy * tx + iyy * ty;
        gx[e] = vx; gy[e] = vy;
        sx += vx; sy += vy;
    }
    if (diag >= 0) { gx[diag] = -sx; gy[diag] = -sy; }
    if (bad || (diag < 0 && e1 > e0)) atomicAdd(status, 1);               // a column out of range, or a row without its diagonal slot
}

// Zeroes n_words 4-byte words.  A kernel, not hipMemsetAsync: in a captured graph that is replayed behind other queued work, the memset node
// of a status word was seen to store a stale byte pattern (0xC9C9C9C9) instead of 0 on the second replay; a kernel node takes its
// arguments from the node itself.
__global__ __launch_bounds__(256) void mesh_zero_kernel(unsigned* p, long long n_words) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (long long)gridDim.x * blockDim.x) p[i] = 0u;
}
inline void ms_zero(void* p, size_t bytes, hipStream_t st) {              // bytes: a multiple of 4
    const long long n_words = (long long)(bytes / 4);
    if (n_words <= 0) return;
    const long long want = (n_words + 255) / 256;
    const unsigned nb = (unsigned)(want < 1024 ? want : 1024);
    DN_LAUNCH(mesh_zero_kernel, dim3(nb, 1, 1), dim3(256, 1, 1), 0, st, (unsigned*)p, n_words);
}

inline bool ms_bad_shape(int n_verts, int n_faces) { return n_verts < 0 || n_faces < 0 || 9LL * n_faces > 2147483647LL; }
inline size_t ms_even(int n_faces) { return ((size_t)n_faces + 1) & ~(size_t)1; }

template <int WIDTH>
int ms_segment_sum(const int64_t* keys, const int64_t* perm, const double* vals, int m, const int64_t* rank, int n_rows, int32_t* rowptr,
                   int32_t* col, double* out, int32_t* count, void* stream) {
    if (m < 0 || n_rows < 0) return 1;   /* hipErrorInvalidValue */
    if (m == 0 && n_rows == 0) return 0;
    const bool csr = rowptr != nullptr;
    if (!out || (csr && (!col || !count))) return 1;
    if (m > 0 && (!keys || !perm || !vals || (csr && !rank))) return 1;
    hipStream_t st = (hipStream_t)stream;
    if (csr) {                                                            // (no key at all: every row is empty)
        ms_zero(rowptr, sizeof(int32_t) * ((size_t)n_rows + 1), st);
        ms_zero(count, sizeof(int32_t), st);
    } else if (n_rows > 0) {
        ms_zero(out, sizeof(double) * (size_t)n_rows * WIDTH, st);
    }
    if (m == 0) return (int)hipGetLastError();
    const unsigned nb = (unsigned)(((long long)m + 255) / 256);
    dn_prof_begin(DN_K_SMALL, st);
    DN_LAUNCH(mesh_segment_sum_kernel<WIDTH>, dim3(nb, 1, 1), dim3(256, 1, 1), 0, st, (const long long*)keys, (const long long*)perm, vals, m,
              (const long long*)rank, n_rows, (int*)rowptr, (int*)col, out, (int*)count);
    dn_prof_end(DN_K_SMALL, st, (double)m * WIDTH, (double)m * (24.0 + 8.0 * WIDTH));
    return (int)hipGetLastError();
}
}  // namespace

extern "C" {

size_t dn_mesh_workspace_bytes(int n_verts, int n_faces) {
    if (ms_bad_shape(n_verts, n_faces)) return 0;
    return (size_t)264 * ms_even(n_faces);                                // keys and values: 9 + 9 + 3 + 12 words of 8 bytes per face
}

int dn_mesh_emit_f32(const float* verts, int n_verts, const int64_t* faces, int n_faces, void* ws, size_t ws_bytes, int32_t* status, void* stream) {
    if (ms_bad_shape(n_verts, n_faces)) return 1;   /* hipErrorInvalidValue */
    if (n_faces == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (!status || !faces || !ws || (n_verts > 0 && !verts)) return 1;
    if (ws_bytes < dn_mesh_workspace_bytes(n_verts, n_faces)) return 1;
    ms_zero(status, sizeof(int32_t), st);
    const size_t fe = ms_even(n_faces);                                   // every array starts on a 16-byte boundary
    unsigned long long* key_l = (unsigned long long*)ws;
    unsigned long long* val_l = key_l + 9 * fe;
    unsigned long long* key_v = val_l + 9 * fe;
    unsigned long long* val_v = key_v + 3 * fe;
    const unsigned nb = (unsigned)(((long long)n_faces + MS_FPB - 1) / MS_FPB);
    dn_prof_begin(DN_K_SMALL, st);
    DN_LAUNCH(mesh_emit_kernel, dim3(nb, 1, 1), dim3(MS_FPB, 1, 1), 0, st, verts, n_verts, (const long long*)faces, n_faces, key_l, val_l, key_v,
              val_v, (int*)status);
    dn_prof_end(DN_K_SMALL, st, (double)n_faces * 120.0, (double)n_faces * (24.0 + 36.0 + 264.0));
    return (int)hipGetLastError();
}

int dn_segment_sum_f64_f64(const int64_t* keys, const int64_t* perm, const double* vals, int m, const int64_t* rank, int n_rows, int32_t* rowptr,
                           int32_t* col, double* out, int32_t* count, void* stream) {
    return ms_segment_sum<1>(keys, perm, vals, m, rank, n_rows, rowptr, col, out, count, stream);
}

int dn_segment_sum4_f64_f64(const int64_t* keys, const int64_t* perm, const double* vals, int m, int n_rows, double* out, void* stream) {
    return ms_segment_sum<4>(keys, perm, vals, m, nullptr, n_rows, nullptr, nullptr, out, nullptr, stream);
}

int dn_mesh_frames_gradients_f64(const float* verts, int n_verts, const int32_t* rowptr, const int32_t* col, int nnz, const double* normals,
                                 double* frames, double* gx, double* gy, int32_t* status, void* stream) {
    if (n_verts < 0 || nnz < 0) return 1;   /* hipErrorInvalidValue */
    if (n_verts == 0) return nnz != 0;
    hipStream_t st = (hipStream_t)stream;
    if (!status || !verts || !rowptr || !normals || !frames || (nnz > 0 && (!col || !gx || !gy))) return 1;
    ms_zero(status, sizeof(int32_t), st);
    const unsigned nb = (unsigned)(((long long)n_verts + 255) / 256);
    dn_prof_begin(DN_K_SMALL, st);
    DN_LAUNCH(mesh_vertex_kernel, dim3(nb, 1, 1), dim3(256, 1, 1), 0, st, verts, n_verts, (const int*)rowptr, (const int*)col, nnz, normals, frames,
              gx, gy, (int*)status);
    dn_prof_end(DN_K_SMALL, st, (double)n_verts * 40.0 + (double)nnz * 40.0, (double)n_verts * (8.0 + 12.0 + 24.0 + 72.0) + (double)nnz * (4.0 + 12.0 + 12.0 + 16.0));
    return (int)hipGetLastError();
}

}  // extern "C"
