// dn_fmap.hip -- the regularised spectral solve of the functional-map layer (compute_correspondence of the reference's
// functional_correspondence experiment) and its closed-form backward.
//
// For spectral coefficients A, B [K, F] of a pair of shapes:  G = A A^T, H = B A^T, and row i of the map C [K, K] is
//     c_i = (G + lam D_i)^-1 H[i, :]^T,    D_i = diag_j (evals_x[j] - evals_y[i])^2
// -- K symmetric positive (semi-)definite K x K systems that share G.  With dC = dL/dC, u_i = (G + lam D_i)^-1 dC[i, :]^T and U the matrix
// of rows u_i^T:  dG = -U^T C,  dA = (dG + dG^T) A + U^T B,  dB = U A.  The backward never forms dG: with X = C A and Y = U A,
//     dB = Y,    dA = U^T (B - X) - C^T Y,
// which is four K x K x F products on a tile of feature columns and needs nothing from any other tile.
//
// Launches.  Forward: gram, solve.  Backward: gram, solve (both right-hand sides through one factorisation), gradients.
//   gram      a workgroup owns 8 rows of G and H of one pair; A and the 8 rows of B go through LDS in chunks of 128 features; thread (r, j)
//             accumulates G[i][j] and H[i][j] of rows i = i0 + r, i0 + r + 4 over f = 0 .. F-1.  G[i][j] and G[j][i] are the same products in
//             the same order: G is symmetric to the bit, and only its lower triangle is stored -- packed, column-major, as the solve holds it.
//   solve     ONE WAVE per (pair, row i), lane r = matrix row r.  The wave copies the packed triangle to LDS (column-major: the lanes of a
//             column step read consecutive doubles), keeps the diagonal of G + lam D_i beside it, factors once by left-looking Cholesky
//             without pivoting -- the forward substitution of its one (backward: two) right-hand sides rides on the same loop -- and ends
//             with the backward substitution: 2 K barriers in all.  At K = 64 a triangle is 16.6 KB: two waves per workgroup keep four
//             workgroups on a CU's 160 KB.  Every loop count depends on K alone, so all waves of a workgroup meet every barrier whatever
//             their data; the wave of a row past K works on a copy of row K - 1 and stores nothing.
//   gradients a workgroup owns 32 feature columns of one pair: U and C (fp64, from the workspace) and the A tile in LDS, X and Y, then dA.
// Arithmetic: fp32 operands are widened at the load and everything after is fp64 (products of two fp32 numbers are exact there); results are
// rounded to fp32 once, at the store.  The backward recomputes G, the factorisations and c_i from A, B and the eigenvalues -- it never reads
// the rounded fp32 C.  Every sum has a fixed order and nothing is accumulated with atomics, so results are bit-identical from run to run.
// A pivot that is not a positive finite number makes its row singular: the factorisation goes on with 1 in its place (no data-dependent
// branch or index anywhere), the row of C is stored as NaN, the pair's flag is raised (the backward stores NaN in all of that pair's dA and
// dB) and the status word, which the gram kernel zeroes, counts the row.  That counter is the one atomic, an integer.
#include "dn_common.h"
#include "../../include/diffnet_hip.h"

#define FM_MAX_K DN_FMAP_MAX_K
#define FM_TRI (FM_MAX_K * (FM_MAX_K + 1) / 2)   /* doubles of a packed triangle */
#define FM_WPB 2                                  /* waves (= rows of C) per workgroup of the solve kernel */
#define FM_GR 8                                   /* rows of G and H per workgroup of the gram kernel */
#define FM_FC 128                                 /* features per staged chunk of the gram kernel */
#define FM_FT 32                                  /* feature columns per workgroup of the gradient kernel */

namespace {
__device__ __forceinline__ double fm_nan() { return __builtin_nan(""); }
// start of column k of a packed column-major lower triangle of order K: entry (r, k), r >= k, lives at fm_col(k, K) + r - k
__device__ __forceinline__ int fm_col(int k, int K) { return k * K - (k * (k - 1)) / 2; }

// grid (P, ceil(K / 8)), 256 threads
__global__ __launch_bounds__(256) void fmap_gram_kernel(const float* DN_RESTRICT A, const float* DN_RESTRICT B, int K, int F, double* G, double* H,
                                                        int* flags, int* status) {
    __shared__ float sa[FM_MAX_K][FM_FC + 1];
    __shared__ float sb[FM_GR][FM_FC + 1];
    const int tid = threadIdx.x, j = tid & 63, r = tid >> 6;
    const long long p = blockIdx.x;
    const int i0 = blockIdx.y * FM_GR;
    const float* Ap = A + p * K * F;
    const float* Bp = B + p * K * F;
    if (blockIdx.y == 0 && tid == 0) {
        flags[p] = 0;
        if (status && p == 0) *status = 0;
    }
    const int ia = i0 + r, ib = i0 + r + 4;
    const int ca = ia < K ? ia : K - 1, cb = ib < K ? ib : K - 1;      // rows past K read a live row and store nothing
    double ga = 0.0, gb = 0.0, ha = 0.0, hb = 0.0;
    for (int f0 = 0; f0 < F; f0 += FM_FC) {
        const int fc = F - f0 < FM_FC ? F - f0 : FM_FC;
        for (int e = tid; e < K * fc; e += 256) {
            const int rr = e / fc, c = e - rr * fc;
            sa[rr][c] = Ap[(long long)rr * F + f0 + c];
        }
        for (int e = tid; e < FM_GR * fc; e += 256) {
            const int rr = e / fc, c = e - rr * fc;
            sb[rr][c] = i0 + rr < K ? Bp[(long long)(i0 + rr) * F + f0 + c] : 0.f;
        }
        __syncthreads();
        if (j < K) {
            for (int c = 0; c < fc; ++c) {
                const double aj = (double)sa[j][c];
                ga += (double)sa[ca][c] * aj;
                gb += (double)sa[cb][c] * aj;
                ha += (double)sb[r][c] * aj;
                hb += (double)sb[r + 4][c] * aj;
            }
        }
        __syncthreads();
    }
    if (j < K) {
        double* Gp = G + p * ((K * (K + 1)) / 2);
        double* Hp = H + p * K * K;
        if (ia < K) { Hp[ia * K + j] = ha; if (j >= ia) Gp[fm_col(ia, K) + j - ia] = ga; }   // G[j][ia] = G[ia][j], to the bit
        if (ib < K) { Hp[ib * K + j] = hb; if (j >= ib) Gp[fm_col(ib, K) + j - ib] = gb; }
    }
}

// grid (P, ceil(K / FM_WPB)), 64 FM_WPB threads.  Gt: the packed triangles the gram kernel wrote.  Forward: C (fp32).  BWD: Cc and U (fp64,
// workspace), right-hand sides H[i, :] and dC[i, :].
template <bool BWD>
__global__ __launch_bounds__(64 * FM_WPB) void fmap_solve_kernel(const double* DN_RESTRICT Gt, const double* DN_RESTRICT H,
                                                                 const float* DN_RESTRICT ex, const float* DN_RESTRICT ey,
                                                                 const float* DN_RESTRICT dC, int K, double lam, float* C, double* Cc, double* U,
                                                                 int* flags, int* status) {
    __shared__ double sm[FM_WPB][FM_TRI];           // G, then column by column L (strictly lower part; the diagonal slots keep G's)
    __shared__ double sd[FM_WPB][FM_MAX_K];         // diagonal of G + lam D_i
    __shared__ double sinv[FM_WPB][FM_MAX_K];       // 1 / L[j][j]
    __shared__ double sb[FM_WPB][2][FM_MAX_K];      // right-hand sides
    __shared__ double sy[FM_WPB][2][FM_MAX_K];      // y = L^-1 b, then x = L^-T y
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const long long p = blockIdx.x;
    const int i_raw = blockIdx.y * FM_WPB + w;
    const bool live = i_raw < K;
    const int i = live ? i_raw : K - 1;
    const bool row = l < K;
    const int tri = (K * (K + 1)) / 2;
    double* M = sm[w];
    const double* Gp = Gt + p * tri;

#pragma unroll 4
    for (int e = l; e < tri; e += 64) M[e] = Gp[e];
    if (row) {
        const double d = (double)ex[p * K + l] - (double)ey[p * K + i];
        sd[w][l] = Gp[fm_col(l, K)] + lam * d * d;
        sb[w][0][l] = H[(p * K + i) * K + l];
        if (BWD) sb[w][1][l] = (double)dC[(p * K + i) * K + l];
    }
    __syncthreads();

    // Left-looking Cholesky, column j of L from columns 0 .. j-1, one barrier per column.  Lane l > j owns L[l][j]; the pivot and entry j
    // of y = L^-1 b are sums over the same L[j][k] every lane reads anyway (one broadcast address), so every lane forms them itself -- the
    // same operations in the same order, the same bits in all lanes -- and the forward substitution costs no pass of its own.  Lanes that
    // own nothing in column j (l <= j, l >= K) run the loop on row j: no lane-dependent branch, every address inside the triangle.
    bool bad = false;
    int cj = 0;                                      // fm_col(j, K)
    for (int j = 0; j < K; ++j) {
        const bool mine = row && l > j;
        const int lr = mine ? l : j;
        double s = M[cj + lr - j];
        double piv = sd[w][j], t1 = sb[w][0][j], t2 = BWD ? sb[w][1][j] : 0.0;
        int ck = 0;
#pragma unroll 4
        for (int k = 0; k < j; ++k) {
            const double bj = M[ck + j - k];
            s -= M[ck + lr - k] * bj;
            piv -= bj * bj;
            t1 -= bj * sy[w][0][k];
            if (BWD) t2 -= bj * sy[w][1][k];
            ck += K - k;
        }
        if (!(piv > 0.0 && piv <= 1.7976931348623157e308)) { bad = true; piv = 1.0; }
        const double inv = 1.0 / sqrt(piv);
        if (mine) M[cj + l - j] = s * inv;
        if (l == 0) {
            sinv[w][j] = inv;
            sy[w][0][j] = t1 * inv;
            if (BWD) sy[w][1][j] = t2 * inv;
        }
        __syncthreads();
        cj += K - j;
    }

    // L^T x = y: lane l carries y_l minus what the rows below have contributed; row j is finished at step j and published through LDS
    double x1 = 0.0, x2 = 0.0;
    if (row) {
        x1 = sy[w][0][l];
        if (BWD) x2 = sy[w][1][l];
    }
    const int cl = row ? fm_col(l, K) - l : 0;       // L[j][l], j > l, lives at cl + j
    for (int j = K - 1; j >= 0; --j) {
        if (l == j) {
            x1 *= sinv[w][j]; sy[w][0][j] = x1;
            if (BWD) { x2 *= sinv[w][j]; sy[w][1][j] = x2; }
        }
        __syncthreads();
        if (l < j) {                                 // (j < K: l is a row)
            const double m = M[cl + j];
            x1 -= m * sy[w][0][j];
            if (BWD) x2 -= m * sy[w][1][j];
        }
    }
    if (!live || !row) return;                       // (the last barrier is behind us)
    if (bad) {
        x1 = fm_nan(); x2 = fm_nan();
        if (l == 0) {
            flags[p] = 1;
            if (status) atomicAdd(status, 1);
        }
    }
    const long long o = (p * K + i) * K + l;
    if (BWD) { Cc[o] = x1; U[o] = x2; }
    else C[o] = (float)x1;
}

// grid (P, ceil(F / FM_FT)), 256 threads: thread (q, f) owns column f of the tile and rows q, q + 8, ...
__global__ __launch_bounds__(256) void fmap_grad_kernel(const float* DN_RESTRICT A, const float* DN_RESTRICT B, const double* DN_RESTRICT Cc,
                                                        const double* DN_RESTRICT U, const int* DN_RESTRICT flags, int K, int F, float* dA,
                                                        float* dB) {
    __shared__ double su[FM_MAX_K][FM_MAX_K];
    __shared__ double sc[FM_MAX_K][FM_MAX_K];
    __shared__ double sw[FM_MAX_K][FM_FT];       // B - X
    __shared__ double sy[FM_MAX_K][FM_FT];       // Y
    __shared__ float sa[FM_MAX_K][FM_FT + 1];
    const int tid = threadIdx.x, f = tid & (FM_FT - 1), q = tid / FM_FT;
    const long long p = blockIdx.x;
    const int f0 = blockIdx.y * FM_FT;
    const int ft = F - f0 < FM_FT ? F - f0 : FM_FT;
    const bool col = f < ft;
    const float* Ap = A + p * K * F;
    const float* Bp = B + p * K * F;
    const bool bad = flags[p] != 0;

    for (int e = tid; e < K * K; e += 256) {
        const int rr = e / K, c = e - rr * K;
        su[rr][c] = U[p * K * K + e];
        sc[rr][c] = Cc[p * K * K + e];
    }
    for (int e = tid; e < K * FM_FT; e += 256) {
        const int rr = e / FM_FT, c = e - rr * FM_FT;
        sa[rr][c] = c < ft ? Ap[(long long)rr * F + f0 + c] : 0.f;
    }
    __syncthreads();
    for (int i = q; i < K; i += 256 / FM_FT) {       // X = C A, Y = U A
        double x = 0.0, y = 0.0;
        for (int k = 0; k < K; ++k) {
            const double a = (double)sa[k][f];
            x += sc[i][k] * a;
            y += su[i][k] * a;
        }
        const double b = col ? (double)Bp[(long long)i * F + f0 + f] : 0.0;
        sw[i][f] = b - x;
        sy[i][f] = y;
        if (col) dB[(p * K + i) * F + f0 + f] = (float)(bad ? fm_nan() : y);
    }
    __syncthreads();
    for (int k = q; k < K; k += 256 / FM_FT) {       // dA = U^T (B - X) - C^T Y
        double g = 0.0;
        for (int i = 0; i < K; ++i) g += su[i][k] * sw[i][f] - sc[i][k] * sy[i][f];
        if (col) dA[(p * K + k) * F + f0 + f] = (float)(bad ? fm_nan() : g);
    }
}

inline size_t fm_mat_bytes(int P, int K) { return (size_t)P * (size_t)K * (size_t)K * sizeof(double); }

// the sizes every entry point checks (F is bounded by the y extent of the gradient kernel's grid); returns 0 when the call may go on
inline int fm_check(int P, int K, int F) { return (K < 1 || K > FM_MAX_K || F < 1 || F > 65535 * FM_FT || P < 0) ? 1 : 0; }

struct fm_ws_t { double *G, *H, *Cc, *U; int* flags; };
inline fm_ws_t fm_carve(void* ws, int P, int K) {
    char* base = (char*)ws + ((256 - ((uintptr_t)ws & 255)) & 255);
    const size_t m = fm_mat_bytes(P, K);
    fm_ws_t o;
    o.G = (double*)base;
    o.H = (double*)(base + m);
    o.Cc = (double*)(base + 2 * m);
    o.U = (double*)(base + 3 * m);
    o.flags = (int*)(base + 4 * m);
    return o;
}
}  // namespace

extern "C" {

int dn_fmap_max_k(void) { return FM_MAX_K; }

size_t dn_fmap_workspace_bytes(int P, int K, int F) {
    if (fm_check(P, K, F) || P == 0) return 0;
    return 4 * fm_mat_bytes(P, K) + (size_t)P * sizeof(int) + 512;   /* G, H, C and U in fp64, one flag per pair, alignment */
}

int dn_fmap_solve_fwd_f32(const float* A, const float* B, const float* evals_x, const float* evals_y, int P, int K, int F, float lam, float* C,
                          void* ws, size_t ws_bytes, int32_t* status, void* stream) {
    if (fm_check(P, K, F)) return 1;   /* hipErrorInvalidValue */
    if (P == 0) return 0;
    if (!A || !B || !evals_x || !evals_y || !C || !ws || ws_bytes < dn_fmap_workspace_bytes(P, K, F)) return 1;
    hipStream_t st = (hipStream_t)stream;
    const fm_ws_t w = fm_carve(ws, P, K);
    const double pk = (double)P * K;
    dn_prof_begin(DN_K_SMALL, st);
    DN_LAUNCH(fmap_gram_kernel, dim3((unsigned)P, (unsigned)((K + FM_GR - 1) / FM_GR), 1), dim3(256, 1, 1), 0, st, A, B, K, F, w.G, w.H, w.flags,
              (int*)status);
    DN_LAUNCH(fmap_solve_kernel<false>, dim3((unsigned)P, (unsigned)((K + FM_WPB - 1) / FM_WPB), 1), dim3(64 * FM_WPB, 1, 1), 0, st, w.G, w.H,
              evals_x, evals_y, (const float*)nullptr, K, (double)lam, C, (double*)nullptr, (double*)nullptr, w.flags, (int*)status);
    dn_prof_end(DN_K_SMALL, st, pk * (4.0 * K * F + K * K * (K / 3.0 + 4.0)), pk * (8.0 * F + 4.0 * K + 8.0 * K * K + 32.0 * K));
    return (int)hipGetLastError();
}

int dn_fmap_solve_bwd_f32(const float* A, const float* B, const float* evals_x, const float* evals_y, const float* dC, int P, int K, int F, float lam,
                          float* dA, float* dB, void* ws, size_t ws_bytes, int32_t* status, void* stream) {
    if (fm_check(P, K, F)) return 1;
    if (P == 0) return 0;
    if (!A || !B || !evals_x || !evals_y || !dC || !dA || !dB || !ws || ws_bytes < dn_fmap_workspace_bytes(P, K, F)) return 1;
    hipStream_t st = (hipStream_t)stream;
    const fm_ws_t w = fm_carve(ws, P, K);
    const double pk = (double)P * K;
    dn_prof_begin(DN_K_SMALL, st);
    DN_LAUNCH(fmap_gram_kernel, dim3((unsigned)P, (unsigned)((K + FM_GR - 1) / FM_GR), 1), dim3(256, 1, 1), 0, st, A, B, K, F, w.G, w.H, w.flags,
              (int*)status);
    DN_LAUNCH(fmap_solve_kernel<true>, dim3((unsigned)P, (unsigned)((K + FM_WPB - 1) / FM_WPB), 1), dim3(64 * FM_WPB, 1, 1), 0, st, w.G, w.H,
              evals_x, evals_y, dC, K, (double)lam, (float*)nullptr, w.Cc, w.U, w.flags, (int*)status);
    DN_LAUNCH(fmap_grad_kernel, dim3((unsigned)P, (unsigned)((F + FM_FT - 1) / FM_FT), 1), dim3(256, 1, 1), 0, st, A, B, (const double*)w.Cc,
              (const double*)w.U, (const int*)w.flags, K, F, dA, dB);
    dn_prof_end(DN_K_SMALL, st, pk * (4.0 * K * F + K * K * (K / 3.0 + 8.0) + 8.0 * K * F),
                pk * (16.0 * F + 4.0 * K + 8.0 * K * K + 64.0 * K + 16.0 * K * ((F + FM_FT - 1) / FM_FT)));
    return (int)hipGetLastError();
}

}  // extern "C"
