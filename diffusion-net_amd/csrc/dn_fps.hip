// dn_fps.hip -- farthest point sampling (geometry.farthest_point_sampling, geometry.py:727-751) with the sample loop on the device.
//
// The algorithm is sequential in the samples: sample s + 1 is the point whose squared distance to the nearest of samples 0 .. s is largest.
// The reference runs it as a Python loop of small torch calls with one host round trip per sample; here the loop never leaves the device.
//
// Arithmetic (bit-exact against the fp32 model of tests/fps_cases.py): d2 = (dx*dx + dy*dy) + dz*dz with dx = x - cx, every product and sum
// rounded on its own (no FMA contraction), min_d = d2 < min_d ? d2 : min_d.  The next sample is the largest min_d, equal values going to the
// lowest index: the order key is (bits of min_d) << 32 | (0xFFFFFFFF - local index) compared as an unsigned 64-bit integer (min_d >= 0, so
// its bit pattern orders like its value).  Keys of different points differ, so the winner does not depend on the order of the reduction and
// both routes below produce the same bits.  The first sample is the point of smallest |p|^2 = (x*x + y*y) + z*z (lowest index among equals)
// -- the same reduction on the complemented bits -- unless the caller names it.
//
// Resident route: one workgroup per cloud, ONE launch.  Point i of the cloud lives in thread i % NT, register slot i / NT, with its min_d;
// per sample every thread updates its P points and forms its best key (and that point's coordinates), the wave reduces the key with
// shuffles, the lane that owns the wave's best leaves (key, x, y, z) in an LDS slot (two slot sets, alternating per sample), one
// __syncthreads(), and every wave reads all slots: the next sample's coordinates never come from global memory.  A one-wave workgroup
// (clouds of up to 64 P points) needs neither LDS nor a barrier: the owner lane is known from the key's index.  Padding slots past the end of
// the cloud hold min_d = 0 with indices above every real point, so they lose every comparison without a validity test in the loop.
//
// Stepped route (clouds past the resident capacity): one launch per sample, a 256-thread workgroup per 1024 points.  A launch first
// reduces the (key, x, y, z) partials the workgroups of the previous launch left in the workspace -- every workgroup does, redundantly;
// workgroup 0 also writes order / radii -- then updates its slice of min_d (kept in the workspace) and leaves its own partial in the other
// parity buffer.  Stream order between the launches is the only synchronisation.
//
// No kernel waits on another workgroup, there are no float atomics, no memsets (the kernels initialise what they read) and no host
// synchronisation.  Every address is formed from thread / block indices, `offsets` and (clamped into the cloud) `start`: point VALUES never
// reach an address, so non-finite coordinates cannot cause an out-of-range access.
#include "dn_common.h"
#include "../../include/diffnet_hip.h"

/* No FMA contraction anywhere in this file, in the device build and in the host build of the emulator alike.  (HIP's __fmul_rn / __fadd_rn
 * do not give that: in this toolchain they are plain operators compiled under hipcc's default -ffp-contract=fast, and were fused.) */
#pragma clang fp contract(off)

#define FPS_PMAX 23                  /* points per thread of the 1024-thread resident kernel: the largest that compiles without scratch (24 spills) */
#define FPS_RESIDENT_MAX (1024 * FPS_PMAX)
#define FPS_STEP_NT 256
#define FPS_STEP_P 4
#define FPS_SLICE (FPS_STEP_NT * FPS_STEP_P)   /* points per workgroup of the stepped route */

#ifdef DN_EMULATE
#define FPS_SCHED_FENCE() do {} while (0)
#else
#define FPS_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#endif

namespace {
typedef unsigned long long fps_u64;

__device__ __forceinline__ float fps_inf() { return __uint_as_float(0x7f800000u); }
// plain operators under the pragma above: each is one correctly rounded fp32 operation
__device__ __forceinline__ float fps_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float fps_add(float a, float b) { return a + b; }
__device__ __forceinline__ float fps_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float fps_norm2(float x, float y, float z) { return fps_add(fps_add(fps_mul(x, x), fps_mul(y, y)), fps_mul(z, z)); }
__device__ __forceinline__ float fps_d2(float x, float y, float z, float cx, float cy, float cz) {
    return fps_norm2(fps_sub(x, cx), fps_sub(y, cy), fps_sub(z, cz));
}
__device__ __forceinline__ fps_u64 fps_key(unsigned hi, unsigned lo) { return ((fps_u64)hi << 32) | lo; }
__device__ __forceinline__ unsigned fps_key_index(fps_u64 key) { return 0xFFFFFFFFu - (unsigned)key; }

__device__ __forceinline__ fps_u64 fps_shfl_xor(fps_u64 v, int mask) {
#ifdef DN_EMULATE   /* the emulator shuffles floats: two halves, as bit patterns */
    const unsigned lo = __float_as_uint(__shfl_xor(__uint_as_float((unsigned)v), mask, 64));
    const unsigned hi = __float_as_uint(__shfl_xor(__uint_as_float((unsigned)(v >> 32)), mask, 64));
    return fps_key(hi, lo);
#else
    return __shfl_xor(v, mask, 64);
#endif
}
__device__ __forceinline__ fps_u64 fps_wave_max(fps_u64 k) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const fps_u64 o = fps_shfl_xor(k, d); k = o > k ? o : k; }
    return k;
}

// The largest key of the workgroup and the coordinates that travel with it, to every thread.  `par` selects the slot set; two consecutive
// calls must use different sets (the second call's writes may overtake a slow wave's reads of the first).  The key of index i is
// presented by thread (i / DIV) % NT -- that is how the winner's slot (NT = 64: lane; no LDS, no barrier) is found without a search.
template <int NT, int DIV = 1>
__device__ __forceinline__ void fps_block_best(fps_u64& key, float& bx, float& by, float& bz, fps_u64 (*skey)[NT / 64], float4 (*sxyz)[NT / 64],
                                               int par) {
    const fps_u64 wk = fps_wave_max(key);
    if (NT == 64) {
        const int owner = (int)((fps_key_index(wk) / (unsigned)DIV) & 63u);
        bx = __shfl(bx, owner, 64);
        by = __shfl(by, owner, 64);
        bz = __shfl(bz, owner, 64);
        key = wk;
        return;
    }
    if (key == wk) {
        skey[par][threadIdx.x >> 6] = wk;
        sxyz[par][threadIdx.x >> 6] = make_float4(bx, by, bz, 0.f);
    }
    __syncthreads();
    // every wave reduces the NT / 64 slots on its own: lane l holds slot l % (NT / 64); the winner's slot follows from its index
    fps_u64 best = skey[par][threadIdx.x & (NT / 64 - 1)];
#pragma unroll
    for (int d = NT / 128; d > 0; d >>= 1) { const fps_u64 o = fps_shfl_xor(best, d); best = o > best ? o : best; }
    const float4 v = sxyz[par][((fps_key_index(best) / (unsigned)DIV) % (unsigned)NT) >> 6];
    key = best; bx = v.x; by = v.y; bz = v.z;
}

// grid (n_clouds): the whole sample loop of one cloud of at most NT * P points.
template <int NT, int P>
__global__ __launch_bounds__(NT) void fps_resident_kernel(const float* DN_RESTRICT pts, const long long* DN_RESTRICT offsets, int n_sample,
                                                          const long long* DN_RESTRICT start, long long* DN_RESTRICT order,
                                                          float* DN_RESTRICT radii, float* DN_RESTRICT min_dist2) {
    __shared__ fps_u64 skey[2][NT / 64];
    __shared__ float4 sxyz[2][NT / 64];
    const int tid = threadIdx.x;
    const int c = blockIdx.x;
    const long long off = offsets[c];
    const long long nn = offsets[c + 1] - off;
    const int n = nn < 0 ? 0 : (nn > (long long)NT * P ? NT * P : (int)nn);   // (the host checked max_points; the clamp keeps a wrong one in bounds)
    long long* ord = order + (long long)c * n_sample;
    float* rad = radii + (long long)c * n_sample;
    if (n == 0) {                                 // an empty cloud has no sample (the host refuses n_sample > min_points)
        for (int s = tid; s < n_sample; s += NT) { ord[s] = -1; rad[s] = 0.f; }
        return;
    }

    float x[P], y[P], z[P], md[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int i = j * NT + tid;
        const bool ok = i < n;
        const float* p = pts + (off + (ok ? i : 0)) * 3;
        x[j] = ok ? p[0] : 0.f;
        y[j] = ok ? p[1] : 0.f;
        z[j] = ok ? p[2] : 0.f;
        md[j] = ok ? fps_inf() : 0.f;
    }

    fps_u64 key;
    float cx, cy, cz;
    if (start) {
        long long s0 = start[c] - off;
        s0 = s0 < 0 ? 0 : (s0 > n - 1 ? n - 1 : s0);
        const float* p = pts + (off + s0) * 3;
        cx = p[0]; cy = p[1]; cz = p[2];
        key = fps_key(0u, 0xFFFFFFFFu - (unsigned)s0);
    } else {                                      // the centremost point: the same reduction on the complemented bits of |p|^2
        unsigned bb = 0, bl = 0;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int i = j * NT + tid;
            const unsigned hb = i < n ? ~__float_as_uint(fps_norm2(x[j], y[j], z[j])) : 0u;
            if (j == 0 || hb > bb) { bb = hb; bl = 0xFFFFFFFFu - (unsigned)i; cx = x[j]; cy = y[j]; cz = z[j]; }
        }
        key = fps_key(bb, bl);
        fps_block_best<NT>(key, cx, cy, cz, skey, sxyz, 1);
    }

    for (int s = 0;; ++s) {
        if (tid == 0) {
            ord[s] = off + (long long)fps_key_index(key);
            rad[s] = s == 0 ? fps_inf() : __uint_as_float((unsigned)(key >> 32));
        }
        const bool last = s == n_sample - 1;
        if (last && !min_dist2) break;
        unsigned bb = 0, bl = 0;
        float bx = 0.f, by = 0.f, bz = 0.f;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const float d = fps_d2(x[j], y[j], z[j], cx, cy, cz);
            const float m = d < md[j] ? d : md[j];
            md[j] = m;
            const unsigned hb = __float_as_uint(m);
            if (j == 0 || hb > bb) { bb = hb; bl = 0xFFFFFFFFu - (unsigned)(j * NT + tid); bx = x[j]; by = y[j]; bz = z[j]; }   // ascending index: strict
            FPS_SCHED_FENCE();                    // one point at a time: interleaving the P chains costs more registers than the wave has
        }
        if (last) break;
        key = fps_key(bb, bl);
        cx = bx; cy = by; cz = bz;
        fps_block_best<NT>(key, cx, cy, cz, skey, sxyz, s & 1);
    }
    if (min_dist2) {
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int i = j * NT + tid;
            if (i < n) min_dist2[off + i] = md[j];
        }
    }
}

// grid (G, n_clouds), launch t = 0 .. n_sample.  t = 0: min_d = inf, partials of the first sample.  t >= 1: sample t - 1 from the partials
// of launch t - 1, then the update against it and (t < n_sample) the partials of sample t.
__global__ __launch_bounds__(FPS_STEP_NT) void fps_step_kernel(const float* DN_RESTRICT pts, const long long* DN_RESTRICT offsets, int n_clouds,
                                                               int n_sample, const long long* DN_RESTRICT start, int t, int G,
                                                               float* DN_RESTRICT md, fps_u64* DN_RESTRICT pkey, float4* DN_RESTRICT pxyz,
                                                               long long* DN_RESTRICT order, float* DN_RESTRICT radii,
                                                               float* DN_RESTRICT min_dist2) {
    __shared__ fps_u64 skey[2][FPS_STEP_NT / 64];
    __shared__ float4 sxyz[2][FPS_STEP_NT / 64];
    const int tid = threadIdx.x;
    const int c = blockIdx.y, g = blockIdx.x;
    const long long off = offsets[c];
    const long long nn = offsets[c + 1] - off;
    const long long cap = (long long)G * FPS_SLICE;
    const int n = nn < 0 ? 0 : (nn > cap ? (int)cap : (int)nn);
    const int nwg = (n + FPS_SLICE - 1) / FPS_SLICE;
    if (n == 0) {
        if (g == 0 && tid == 0 && t >= 1) { order[(long long)c * n_sample + t - 1] = -1; radii[(long long)c * n_sample + t - 1] = 0.f; }
        return;
    }
    if (g >= nwg) return;
    const int i0 = g * FPS_SLICE;
    float* mdc = md + (size_t)c * (size_t)G * FPS_SLICE;   // this cloud's min_d: a stride of whole slices of the largest cloud
    unsigned bb = 0, bl = 0;
    float bx = 0.f, by = 0.f, bz = 0.f;

    if (t == 0) {
        long long s0 = -1;
        if (start) { s0 = start[c] - off; s0 = s0 < 0 ? 0 : (s0 > n - 1 ? n - 1 : s0); }
#pragma unroll
        for (int j = 0; j < FPS_STEP_P; ++j) {
            const int i = i0 + j * FPS_STEP_NT + tid;
            const bool ok = i < n;
            float px = 0.f, py = 0.f, pz = 0.f;
            unsigned hb = 0u;
            if (ok) {
                const float* p = pts + (off + i) * 3;
                px = p[0]; py = p[1]; pz = p[2];
                mdc[i] = fps_inf();
                hb = start ? (i == s0 ? 0xFFFFFFFFu : 0u) : ~__float_as_uint(fps_norm2(px, py, pz));
            }
            if (j == 0 || hb > bb) { bb = hb; bl = 0xFFFFFFFFu - (unsigned)i; bx = px; by = py; bz = pz; }
        }
    } else {
        const fps_u64* pk = pkey + ((size_t)((t - 1) & 1) * n_clouds + c) * G;
        const float4* px4 = pxyz + ((size_t)((t - 1) & 1) * n_clouds + c) * G;
        fps_u64 key = 0;
        float cx = 0.f, cy = 0.f, cz = 0.f;
        for (int q = tid; q < nwg; q += FPS_STEP_NT) {
            const fps_u64 k = pk[q];
            if (k > key) { const float4 v = px4[q]; key = k; cx = v.x; cy = v.y; cz = v.z; }
        }
        fps_block_best<FPS_STEP_NT, FPS_SLICE>(key, cx, cy, cz, skey, sxyz, 0);   // partial q = the slice of points q * FPS_SLICE ..
        if (g == 0 && tid == 0) {
            order[(long long)c * n_sample + t - 1] = off + (long long)fps_key_index(key);
            radii[(long long)c * n_sample + t - 1] = t == 1 ? fps_inf() : __uint_as_float((unsigned)(key >> 32));
        }
        const bool last = t == n_sample;
        if (last && !min_dist2) return;
#pragma unroll
        for (int j = 0; j < FPS_STEP_P; ++j) {
            const int i = i0 + j * FPS_STEP_NT + tid;
            const bool ok = i < n;
            float px = 0.f, py = 0.f, pz = 0.f, m = 0.f;
            if (ok) {
                const float* p = pts + (off + i) * 3;
                px = p[0]; py = p[1]; pz = p[2];
                const float d = fps_d2(px, py, pz, cx, cy, cz);
                const float old = mdc[i];
                m = d < old ? d : old;
                mdc[i] = m;
                if (last) min_dist2[off + i] = m;
            }
            const unsigned hb = __float_as_uint(m);
            if (j == 0 || hb > bb) { bb = hb; bl = 0xFFFFFFFFu - (unsigned)i; bx = px; by = py; bz = pz; }
        }
        if (last) return;
    }
    fps_u64 key = fps_key(bb, bl);
    fps_block_best<FPS_STEP_NT>(key, bx, by, bz, skey, sxyz, 1);
    if (tid == 0) {
        pkey[((size_t)(t & 1) * n_clouds + c) * G + g] = key;
        pxyz[((size_t)(t & 1) * n_clouds + c) * G + g] = make_float4(bx, by, bz, 0.f);
    }
}

inline int fps_step_groups(int max_points) { const int g = (int)(((long long)max_points + FPS_SLICE - 1) / FPS_SLICE); return g < 1 ? 1 : g; }
inline size_t fps_align256(size_t b) { return (b + 255) & ~(size_t)255; }
// 0: nothing fits, 1: resident, 2: stepped
inline int fps_resolve_route(int max_points, int route) {
    if (route == 0) return max_points <= FPS_RESIDENT_MAX ? 1 : 2;
    if (route == 1) return max_points <= FPS_RESIDENT_MAX ? 1 : 0;
    return route == 2 ? 2 : 0;
}
// partials of both parities, then min_d [n_clouds][G * FPS_SLICE] (a stride the call can check: the total of a ragged batch is not its argument)
inline size_t fps_step_ws_bytes(int n_clouds, int max_points) {
    const size_t G = (size_t)fps_step_groups(max_points), parts = 2 * (size_t)n_clouds * G;
    return fps_align256(parts * sizeof(fps_u64)) + fps_align256(parts * sizeof(float4)) + (size_t)n_clouds * G * FPS_SLICE * sizeof(float) + 256;
}
}  // namespace

#define FPS_RESIDENT_LAUNCH(NT_, P_)                                                                                              \
    DN_LAUNCH((fps_resident_kernel<NT_, P_>), dim3((unsigned)n_clouds, 1, 1), dim3(NT_, 1, 1), 0, stream, pts, offsets, n_sample, \
              start, order, radii, min_dist2)

int dn_launch_fps_resident(const float* pts, const long long* offsets, int n_clouds, int max_points, int n_sample, const long long* start,
                           long long* order, float* radii, float* min_dist2, hipStream_t stream) {
    dn_prof_begin(DN_K_SMALL, stream);
    if (max_points <= 64 * 8) FPS_RESIDENT_LAUNCH(64, 8);
    else if (max_points <= 256 * 8) FPS_RESIDENT_LAUNCH(256, 8);
    else if (max_points <= 1024 * 8) FPS_RESIDENT_LAUNCH(1024, 8);
    else FPS_RESIDENT_LAUNCH(1024, FPS_PMAX);
    dn_prof_end(DN_K_SMALL, stream, 9.0 * (double)n_clouds * max_points * n_sample, 12.0 * (double)n_clouds * max_points);
    return (int)hipGetLastError();
}

int dn_launch_fps_stepped(const float* pts, const long long* offsets, int n_clouds, int max_points, int n_sample, const long long* start,
                          float* md, void* pkey, void* pxyz, long long* order, float* radii, float* min_dist2, hipStream_t stream) {
    const int G = fps_step_groups(max_points);
    dn_prof_begin(DN_K_SMALL, stream);
    for (int t = 0; t <= n_sample; ++t)
        DN_LAUNCH(fps_step_kernel, dim3((unsigned)G, (unsigned)n_clouds, 1), dim3(FPS_STEP_NT, 1, 1), 0, stream, pts, offsets, n_clouds, n_sample,
                  start, t, G, md, (fps_u64*)pkey, (float4*)pxyz, order, radii, min_dist2);
    dn_prof_end(DN_K_SMALL, stream, 9.0 * (double)n_clouds * max_points * n_sample, 20.0 * (double)n_clouds * max_points * n_sample);
    return (int)hipGetLastError();
}

extern "C" {

int dn_fps_resident_max_points(void) { return FPS_RESIDENT_MAX; }

size_t dn_fps_workspace_bytes(int64_t n_points_total, int n_clouds, int max_points, int n_sample, int route) {
    (void)n_sample;
    if (n_points_total <= 0 || n_clouds <= 0 || max_points <= 0) return 0;
    if (fps_resolve_route(max_points, route) != 2) return 0;
    return fps_step_ws_bytes(n_clouds, max_points);
}

int dn_fps_f32(const float* pts, const int64_t* offsets, int n_clouds, int min_points, int max_points, int n_sample, const int64_t* start,
               int route, int64_t* order, float* radii, float* min_dist2, void* ws, size_t ws_bytes, void* stream) {
    if (n_clouds < 0 || n_sample < 1 || n_sample > min_points || max_points < min_points) return 1;   /* hipErrorInvalidValue */
    const int r = fps_resolve_route(max_points, route);
    if (r == 0) return 1;
    if (n_clouds == 0) return 0;
    if (!pts || !offsets || !order || !radii) return 1;
    if (r == 1)
        return dn_launch_fps_resident(pts, (const long long*)offsets, n_clouds, max_points, n_sample, (const long long*)start, (long long*)order,
                                      radii, min_dist2, (hipStream_t)stream);
    if (n_clouds > 65535) return 1;                                        /* grid.y */
    if (!ws || ws_bytes < fps_step_ws_bytes(n_clouds, max_points)) return 1;
    const size_t parts = 2 * (size_t)n_clouds * (size_t)fps_step_groups(max_points);
    char* base = (char*)ws + ((256 - ((uintptr_t)ws & 255)) & 255);
    void* pkey = base;
    void* pxyz = base + fps_align256(parts * sizeof(fps_u64));
    float* md = (float*)(base + fps_align256(parts * sizeof(fps_u64)) + fps_align256(parts * sizeof(float4)));
    return dn_launch_fps_stepped(pts, (const long long*)offsets, n_clouds, max_points, n_sample, (const long long*)start, md, pkey, pxyz,
                                 (long long*)order, radii, min_dist2, (hipStream_t)stream);
}

}  // extern "C"
