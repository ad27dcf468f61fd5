// dn_eigen.hip -- one step of the Chebyshev three-term recurrence on a block of vectors (ops.cheb_step; the products with S of the filtered
// subspace iteration of geometry.laplacian_eigenbasis):
//
//     out[i][c] = alpha * sum_p val[p] * Y[col[p]][c]  +  beta * Y[i][c]  +  gamma * Z[i][c]      p in [rowptr[i], rowptr[i + 1])
//
// S is CSR (int32 rowptr / col, fp64 val), the blocks are fp64 row-major [n_rows][ld] of which columns [0, nb) are used.  (1, 0, 0) is the
// plain product S X; (2 / e, -2 c / e, -1) with Z the block before last is  T_(j+1) = 2 ((S - c) / e) T_j - T_(j-1).
//
// Shape: the access pattern of dn_geodesic.hip with (+, *) in place of (min, +).  The 64 lanes of a wave are 64 consecutive columns, a wave
// owns one row at a time, so a neighbour's row segment is ONE contiguous 512-byte read and the row's entries (col, val) are the same for every
// lane -- the row index is made wave-uniform, which turns rowptr / col / val into scalar loads.  256 threads = 4 waves; a workgroup owns
// CH_ROWS consecutive rows (CH_RPW per wave) of one 64-column tile; any nb by column tiles (blockIdx.y), the lanes past nb read and write
// nothing.  blockIdx.x walks the row tiles fastest and every XCD a contiguous range of them, so the workgroups in flight share a column
// tile: its n_rows x 512 bytes are what the caches hold.
//
// Rows per workgroup: nothing is staged and no lane waits for another, so a row costs its chain of dependent reads (rowptr -> col / val ->
// the neighbours' segments) and only other waves hide it.  The entries of a row are taken CH_CHUNK at a time: 8 segment reads of 8 bytes per
// lane, 4 KiB per wave, are in flight per step, and at the 24 VGPRs this needs a CU holds 32 waves = 128 KiB of reads, several times what
// hides a miss to HBM.  Occupancy is therefore not the limit and the rows per wave are kept SMALL (2): the block of a 2 000-vertex mesh is
// then 750 workgroups, about three per CU, where 4 rows per wave would leave a third of the CUs with one.
//
// Arithmetic: one fp64 fma per entry, in CSR order, nothing reassociated, no atomics: results are repeatable bit for bit.  A term whose
// scalar is 0 is not formed (beta == 0: Y[i] is not read for it; gamma == 0: Z is not read and may be NULL), as in BLAS.  Every element of
// out is written by the lane that read Y[i][c] and Z[i][c], and no lane reads another's Z: out may be Z.  out must not be Y (other rows of
// Y are read while out is written).  Columns [nb, ld) are never read from Y or Z and never written in out.
#include "dn_common.h"
#include "../../include/diffnet_hip.h"

#define CH_WAVES 4
#define CH_RPW 2                         /* rows per wave */
#define CH_ROWS (CH_WAVES * CH_RPW)      /* rows per workgroup: dn_cheb_rows_per_workgroup() */
#define CH_CHUNK 8                       /* entries gathered per step */

namespace {
__device__ __forceinline__ int ch_uniform(int v) {
#ifdef DN_EMULATE
    return v;
#else
    return __builtin_amdgcn_readfirstlane(v);
#endif
}

// grid (row tiles rounded up to a multiple of 8, 64-column tiles)
__global__ __launch_bounds__(256) void cheb_step_kernel(const int* DN_RESTRICT rowptr, const int* DN_RESTRICT col, const double* DN_RESTRICT val,
                                                        int n_rows, const double* DN_RESTRICT Y, const double* Z, double* out, int nb, size_t ld,
                                                        double alpha, double beta, double gamma) {
    const int lane = threadIdx.x & 63;
    const int wave = ch_uniform((int)(threadIdx.x >> 6));
    const int per_xcd = (int)(gridDim.x >> 3);                    // block b runs on XCD b % 8: each XCD a contiguous range of row tiles
    const long long tile = (long long)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    const long long c = (long long)blockIdx.y * 64 + lane;
    if (c >= nb) return;                                          // ragged nb: the lanes past the end read and write nothing (no barrier below)
#pragma unroll
    for (int r = 0; r < CH_RPW; ++r) {
        const long long v = tile * CH_ROWS + (long long)wave * CH_RPW + r;
        if (v >= n_rows) break;                                   // uniform per wave
        const int beg = rowptr[v], end = rowptr[v + 1];
        double acc = 0.0;
        for (int j0 = beg; j0 < end; j0 += CH_CHUNK) {            // an empty row: acc stays 0
            double yv[CH_CHUNK], sv[CH_CHUNK];
#pragma unroll
            for (int u = 0; u < CH_CHUNK; ++u) {                  // branch-free reads: the slots past the row's end repeat its last entry
                const int j = j0 + u < end ? j0 + u : end - 1;
                sv[u] = val[j];
                yv[u] = Y[(size_t)col[j] * ld + (size_t)c];
            }
#pragma unroll
            for (int u = 0; u < CH_CHUNK; ++u)
                acc = j0 + u < end ? fma(sv[u], yv[u], acc) : acc;   // uniform condition: a repeated entry is not summed
        }
        const size_t at = (size_t)v * ld + (size_t)c;
        double res = alpha * acc;
        if (beta != 0.0) res = fma(beta, Y[at], res);
        if (gamma != 0.0) res = fma(gamma, Z[at], res);
        out[at] = res;
    }
}
}  // namespace

extern "C" {

int dn_cheb_rows_per_workgroup(void) { return CH_ROWS; }

int dn_cheb_step_f64(const int32_t* rowptr, const int32_t* col, const double* val, int n_rows, const double* Y, const double* Z, double* out,
                     int nb, int ld, double alpha, double beta, double gamma, void* stream) {
    if (n_rows < 0 || nb < 0 || ld < nb) return 1;                        /* hipErrorInvalidValue */
    if (!rowptr || !col || !val || !Y || !out || out == Y) return 1;
    if (gamma != 0.0 && !Z) return 1;
    if (n_rows == 0 || nb == 0) return 0;
    const long long tiles = ((long long)n_rows + CH_ROWS - 1) / CH_ROWS;
    const long long groups = ((long long)nb + 63) / 64;
    if (groups > 65535) return 1;                                         /* grid.y */
    const dim3 grid((unsigned)((tiles + 7) / 8 * 8), (unsigned)groups, 1);
    DN_LAUNCH(cheb_step_kernel, grid, dim3(256, 1, 1), 0, (hipStream_t)stream, rowptr, col, val, n_rows, Y, Z, out, nb, (size_t)ld, alpha, beta,
              gamma);
    return (int)hipGetLastError();
}

}  // extern "C"
