// dn_knn.hip -- exact brute-force k-nearest-neighbour search (geometry.find_knn, geometry.py:667-724) that never forms the N x M matrix.
//
// Distances are the DIFFERENCE form the reference uses: d2 = sum_d (a_d - b_d)^2, one fmaf chain per pair in the order d = 0 .. D-1, one
// sqrtf on output.  The chain of a pair runs in one thread and does not depend on where the pair falls in a tile or on how the targets are
// split, so the squared distance of a pair is the same bits in every launch geometry.  The order key is that squared distance (negated for
// `largest`); equal keys go to the lower target index.  (key, index) is a total order, so the k best of a row are ONE set whichever way the
// targets are cut into slices: the result is bit-identical across n_split.
//
// Shape: a 256-thread workgroup owns 64 queries and one contiguous slice of the targets.  64-target tiles are staged through LDS in chunks of
// 32 dimensions (rows padded to 33 words: the 16 target rows a wave reads at once fall on 16 banks, the 4 query rows are broadcasts).  Thread
// (tq, tt) accumulates the 4 x 4 pairs of queries 4 tq + i and targets tt + 16 e in registers.
//   k > 1: every query keeps a sorted k-slot list of (key, index) in LDS (slot-major: lane q on bank q) and its k-th key as a rejection
//          threshold.  A pair that does not beat the threshold costs one compare; one that may is parked in a 64 x 64 key tile with one bit of
//          the query's 64-bit mask.  After the tile, thread q walks the set bits of its mask in ascending order -- insertions of a query happen
//          in ascending target index, so a strict compare resolves ties to the lower index.
//   k = 1: running (key, index) of each of the thread's 4 queries in registers; the 16 threads of a query are merged once, at the end.
// Split-M: with too few query tiles to fill the device the targets are cut into n_split slices; every (query tile, slice) workgroup writes its
// sorted partial list to the workspace (query-fastest: coalesced both ways) and a second kernel merges the slices of a query in slice order
// with the same insertion rule.
#include "dn_common.h"
#include "../../include/diffnet_hip.h"

#define KNN_QT 64            /* queries per workgroup */
#define KNN_TT 64            /* targets per tile */
#define KNN_DC 32            /* dimensions per staged chunk */
#define KNN_LD (KNN_DC + 1)  /* padded row of a staged chunk */
#define KNN_MAX_K DN_KNN_MAX_K
#define KNN_TARGET_WGS 1024  /* automatic n_split: about this many workgroups (256 CUs x 3-4 resident), slices of at least 8 tiles */
#define KNN_MIN_SLICE_TILES 8

namespace {
__device__ __forceinline__ float knn_inf() { return __uint_as_float(0x7f800000u); }

// Insert (key, j) into the sorted list of query column `q` (slot-major arrays).  Callers present the candidates of a query in ascending j, so
// every entry already in the list has a lower index and an equal key must stay in front: strict compares on both sides.
// Returns false when the candidate was rejected by the full list.
__device__ __forceinline__ bool knn_insert(float (*lk)[KNN_QT], int (*li)[KNN_QT], int q, int k, int& cnt, float key, int j) {
    if (cnt == k && !(key < lk[k - 1][q])) return false;
    int p = cnt < k ? cnt : k - 1;
    while (p > 0 && lk[p - 1][q] > key) {
        lk[p][q] = lk[p - 1][q];
        li[p][q] = li[p - 1][q];
        --p;
    }
    lk[p][q] = key;
    li[p][q] = j;
    if (cnt < k) ++cnt;
    return true;
}

// The finished lists of a workgroup's queries -> dist / idx rows q0 .. q0 + nq - 1 (contiguous in memory: every thread of the block takes part).
__device__ __forceinline__ void knn_write_rows(float (*lk)[KNN_QT], int (*li)[KNN_QT], long long q0, int nq, int k, float sgn, float* dist,
                                               long long* idx) {
    const int total = nq * k;
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
        const int q = i / k, e = i - q * k;
        dist[q0 * k + i] = sqrtf(sgn * lk[e][q]);
        idx[q0 * k + i] = (long long)li[e][q];
    }
}

// grid (query tiles, slices).  n_split == 1: dist / idx are written; otherwise the partial lists pk / pi [slice][k][N] (index -1: empty slot).
template <bool K1>
__global__ __launch_bounds__(256) void knn_tile_kernel(const float* DN_RESTRICT src, const float* DN_RESTRICT tgt, int N, int M, int D, int k,
                                                       float sgn, int omit, int tiles_per_slice, int n_split, float* dist, long long* idx,
                                                       float* pk, int* pi) {
    __shared__ float sq[KNN_QT][KNN_LD];
    __shared__ float st[KNN_TT][KNN_LD];
    __shared__ float lk[KNN_MAX_K][KNN_QT];      // k = 1: the 16 per-thread minima of every query, [tt][q] (tt < 16)
    __shared__ int li[KNN_MAX_K][KNN_QT];
    __shared__ float sd[K1 ? 1 : KNN_QT][K1 ? 1 : KNN_TT + 1];
    __shared__ int smask[K1 ? 1 : KNN_QT][2];
    __shared__ float sthr[K1 ? 1 : KNN_QT];

    const int tid = threadIdx.x, tq = tid >> 4, tt = tid & 15;
    const long long q0 = (long long)blockIdx.x * KNN_QT;
    const int nq = (int)((long long)N - q0 < KNN_QT ? (long long)N - q0 : KNN_QT);
    const int slice = blockIdx.y;
    const int n_tiles = (int)(((long long)M + KNN_TT - 1) / KNN_TT);
    const int tile_lo = slice * tiles_per_slice;
    const int tile_hi = tile_lo + tiles_per_slice < n_tiles ? tile_lo + tiles_per_slice : n_tiles;
    const bool one_chunk = D <= KNN_DC;

    int cnt = 0;                                  // list fill of query `tid` (threads 0..63, k > 1)
    float best[4];                                // k = 1: running minimum of the thread's 4 queries over its own targets
    int bidx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { best[i] = knn_inf(); bidx[i] = -1; }
    if (!K1 && tid < KNN_QT) { smask[tid][0] = 0; smask[tid][1] = 0; sthr[tid] = knn_inf(); }
    if (one_chunk) {                              // the queries are staged once
        for (int i = tid; i < KNN_QT * D; i += 256) {
            const int r = i / D, c = i - r * D;
            sq[r][c] = r < nq ? src[(q0 + r) * D + c] : 0.f;
        }
    }

    for (int tile = tile_lo; tile < tile_hi; ++tile) {
        const long long t0 = (long long)tile * KNN_TT;
        const int nt = (int)((long long)M - t0 < KNN_TT ? (long long)M - t0 : KNN_TT);
        float acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][e] = 0.f;

        for (int d0 = 0; d0 < D; d0 += KNN_DC) {
            const int dc = D - d0 < KNN_DC ? D - d0 : KNN_DC;
            for (int i = tid; i < KNN_TT * dc; i += 256) {
                const int r = i / dc, c = i - r * dc;
                st[r][c] = r < nt ? tgt[(t0 + r) * D + d0 + c] : 0.f;
            }
            if (!one_chunk) {
                for (int i = tid; i < KNN_QT * dc; i += 256) {
                    const int r = i / dc, c = i - r * dc;
                    sq[r][c] = r < nq ? src[(q0 + r) * D + d0 + c] : 0.f;
                }
            }
            __syncthreads();                      // chunk staged; the previous tile's insertions (thresholds, cleared masks) are visible
#pragma unroll 2
            for (int d = 0; d < dc; ++d) {
                float a[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = sq[4 * tq + i][d];
#pragma unroll
                for (int e = 0; e < 4; ++e) b[e] = st[tt + 16 * e][d];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float df = a[i] - b[e];
                        acc[i][e] = fmaf(df, df, acc[i][e]);
                    }
            }
            if (d0 + KNN_DC >= D) {               // last chunk: the pairs of this tile are complete
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int ql = 4 * tq + i;
                    const long long qg = q0 + ql;
                    float thr = knn_inf();
                    if (!K1) thr = sthr[ql];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int jl = tt + 16 * e;
                        const long long jg = t0 + jl;
                        if (ql >= nq || jl >= nt || (omit && jg == qg)) continue;
                        const float key = sgn * acc[i][e];
                        if (K1) {                 // the thread meets its targets in ascending index: strict compare keeps the lower one
                            if (key < best[i] || bidx[i] < 0) { best[i] = key; bidx[i] = (int)jg; }
                        } else if (key <= thr) {
                            sd[ql][jl] = key;
                            atomicOr(&smask[ql][jl >> 5], (int)(1u << (jl & 31)));
                        }
                    }
                }
            }
            __syncthreads();                      // every read of the staged chunk is done; parked candidates are visible
        }
        if (!K1 && tid < nq) {
            bool changed = false;
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                unsigned m = (unsigned)smask[tid][w];
                if (m) smask[tid][w] = 0;
                while (m) {
                    const int jl = 32 * w + __builtin_ctz(m);
                    m &= m - 1;
                    changed |= knn_insert(lk, li, tid, k, cnt, sd[tid][jl], (int)(t0 + jl));
                }
            }
            if (changed && cnt == k) sthr[tid] = lk[k - 1][tid];
        }
    }

    if (K1) {                                     // merge the 16 threads of every query: lowest (key, index)
#pragma unroll
        for (int i = 0; i < 4; ++i) { lk[tt][4 * tq + i] = best[i]; li[tt][4 * tq + i] = bidx[i]; }
        __syncthreads();
        if (tid < nq) {
            float bk = knn_inf();
            int bj = -1;
            for (int t = 0; t < 16; ++t) {
                const float key = lk[t][tid];
                const int j = li[t][tid];
                if (j >= 0 && (bj < 0 || key < bk || (key == bk && j < bj))) { bk = key; bj = j; }
            }
            lk[0][tid] = bk; li[0][tid] = bj;     // (slot 0 of column tid was this thread's to read: t = 0 is consumed above)
        }
    }
    if (n_split == 1) {
        __syncthreads();
        knn_write_rows(lk, li, q0, nq, k, sgn, dist, idx);
    } else if (tid < nq) {
        const long long col = q0 + tid;
        const int have = K1 ? (li[0][tid] >= 0 ? 1 : 0) : cnt;
        for (int e = 0; e < k; ++e) {
            const long long o = ((long long)slice * k + e) * N + col;
            pk[o] = e < have ? lk[e][tid] : knn_inf();
            pi[o] = e < have ? li[e][tid] : -1;
        }
    }
}

// One thread per query: the slices' partial lists, in slice order (= ascending target index among equal keys), through the same insertion.
__global__ __launch_bounds__(64) void knn_merge_kernel(const float* DN_RESTRICT pk, const int* DN_RESTRICT pi, int N, int k, int n_split, float sgn,
                                                       float* dist, long long* idx) {
    __shared__ float lk[KNN_MAX_K][KNN_QT];
    __shared__ int li[KNN_MAX_K][KNN_QT];
    const int tid = threadIdx.x;
    const long long q0 = (long long)blockIdx.x * KNN_QT;
    const int nq = (int)((long long)N - q0 < KNN_QT ? (long long)N - q0 : KNN_QT);
    if (tid < nq) {
        int cnt = 0;
        for (int s = 0; s < n_split; ++s)
            for (int e = 0; e < k; ++e) {
                const long long o = ((long long)s * k + e) * N + q0 + tid;
                const int j = pi[o];
                if (j < 0 || !knn_insert(lk, li, tid, k, cnt, pk[o], j)) break;   // a slice's list is sorted: what follows a reject is rejected too
            }
    }
    __syncthreads();
    knn_write_rows(lk, li, q0, nq, k, sgn, dist, idx);
}

inline int knn_tiles(int n_tgt) { return (int)(((long long)n_tgt + KNN_TT - 1) / KNN_TT); }
inline long long knn_qtiles(int n_src) { return ((long long)n_src + KNN_QT - 1) / KNN_QT; }

// the number of target slices of a call and the tiles of each: n_split = 0 fills the device, a forced value is clamped to the tile count;
// either way no slice is empty
inline int knn_resolve_split(int n_src, int n_tgt, int n_split, int* tiles_per_slice) {
    const int n_tiles = knn_tiles(n_tgt);
    long long want = n_split;
    if (want <= 0) {
        const long long qt = knn_qtiles(n_src);
        want = (KNN_TARGET_WGS + qt - 1) / qt;
        const long long cap = n_tiles / KNN_MIN_SLICE_TILES;
        if (want > cap) want = cap;
    }
    if (want > n_tiles) want = n_tiles;
    if (want > 65535) want = 65535;                                       /* grid.y */
    if (want < 1) want = 1;
    const int tps = (int)((n_tiles + want - 1) / want);
    *tiles_per_slice = tps;
    return (n_tiles + tps - 1) / tps;
}
inline size_t knn_partial_floats(int n_src, int k, int n_split) { return (size_t)n_split * (size_t)k * (size_t)n_src; }
}  // namespace

int dn_launch_knn(const float* src, int n_src, const float* tgt, int n_tgt, int dim, int k, int largest, int omit_diagonal, int n_split,
                  int tiles_per_slice, float* dist, long long* idx, float* pk, int* pi, hipStream_t stream) {
    const float sgn = largest ? -1.f : 1.f;
    const dim3 grid((unsigned)knn_qtiles(n_src), (unsigned)n_split, 1);
    const double pairs = (double)n_src * (double)n_tgt;
    dn_prof_begin(DN_K_SMALL, stream);
    if (k == 1)
        DN_LAUNCH(knn_tile_kernel<true>, grid, dim3(256, 1, 1), 0, stream, src, tgt, n_src, n_tgt, dim, k, sgn, omit_diagonal, tiles_per_slice,
                  n_split, dist, idx, pk, pi);
    else
        DN_LAUNCH(knn_tile_kernel<false>, grid, dim3(256, 1, 1), 0, stream, src, tgt, n_src, n_tgt, dim, k, sgn, omit_diagonal, tiles_per_slice,
                  n_split, dist, idx, pk, pi);
    if (n_split > 1)
        DN_LAUNCH(knn_merge_kernel, dim3((unsigned)knn_qtiles(n_src), 1, 1), dim3(64, 1, 1), 0, stream, pk, pi, n_src, k, n_split, sgn, dist, idx);
    dn_prof_end(DN_K_SMALL, stream, 3.0 * pairs * dim, 4.0 * ((double)n_src * dim + (double)knn_qtiles(n_src) * n_tgt * dim + 3.0 * (double)n_src * k));
    return (int)hipGetLastError();
}

extern "C" {

int dn_knn_max_k(void) { return KNN_MAX_K; }

size_t dn_knn_workspace_bytes(int n_src, int n_tgt, int dim, int k, int n_split) {
    (void)dim;
    if (n_src <= 0 || n_tgt <= 0 || k < 1) return 0;
    int tps;
    const int ns = knn_resolve_split(n_src, n_tgt, n_split, &tps);
    if (ns <= 1) return 0;
    return knn_partial_floats(n_src, k, ns) * (sizeof(float) + sizeof(int)) + 512;
}

int dn_knn_f32(const float* src, int n_src, const float* tgt, int n_tgt, int dim, int k, int largest, int omit_diagonal, int n_split,
               float* dist, int64_t* idx, void* ws, size_t ws_bytes, void* stream) {
    if (n_src < 0 || n_tgt < 0 || n_split < 0 || k < 1 || k > KNN_MAX_K || dim < 1) return 1;   /* hipErrorInvalidValue */
    if (omit_diagonal && n_src != n_tgt) return 1;
    if ((long long)k > (long long)n_tgt - (omit_diagonal ? 1 : 0)) return 1;
    if (n_src == 0) return 0;
    if (!src || !tgt || !dist || !idx) return 1;
    int tps;
    const int ns = knn_resolve_split(n_src, n_tgt, n_split, &tps);
    float* pk = nullptr;
    int* pi = nullptr;
    if (ns > 1) {
        if (!ws || ws_bytes < dn_knn_workspace_bytes(n_src, n_tgt, dim, k, n_split)) return 1;
        const size_t mis = (256 - ((uintptr_t)ws & 255)) & 255;
        pk = (float*)((char*)ws + mis);
        pi = (int*)(pk + knn_partial_floats(n_src, k, ns));
    }
    return dn_launch_knn(src, n_src, tgt, n_tgt, dim, k, largest != 0, omit_diagonal != 0, ns, tps, dist, (long long*)idx, pk, pi,
                         (hipStream_t)stream);
}

}  // extern "C"
