// dn_diffuse.hip -- the back-projection of LearnedTimeDiffusion, method='spectral' (layers.py:44-67 + geometry.py:572-598), at K = C = 128 as
// a launch of its own, and the host arithmetic of its work plan:
//     forward   x_diffuse = Phi ys                       ys = exp(-lambda t) * (Phi^T (M x)), the scaled spectrum
//     backward  d_x = add + M * (Phi ys)                 ys = exp(-lambda t) * (Phi^T d_xd)
// The projection and the spectral step in front of it are the split-V kernel of dn_tngemm.hip and the per-mesh reduce of dn_pointwise.hip;
// dn_api.hip (DiffuseRoute.direct) takes this kernel for batches that carry a plan and the row GEMM otherwise.  The kernel began as the third
// phase of round 5's one-launch form of the whole operator, which was measured slower than the three launches and is archived, with its
// numbers, under tools/experiments/diffusion_one_launch/.
#include "dn_tn_tiles.h"
#include "dn_direct_tiles.h"
#include <string.h>

#if defined(DN_DF_TRACE) && !defined(DN_EMULATE)   // development build only (tools/kbench --trace prints the timeline)
__device__ unsigned long long dn_df_wg_times[512 * 2];   // s_memrealtime (100 MHz, chip-wide) at the start / end of every workgroup of backproject_kernel
extern "C" int dn_debug_df_wg_times_read(unsigned long long* out, int n) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(dn_df_wg_times), sizeof(unsigned long long) * n); }
#define DF_WG(i_) do { if (threadIdx.x == 0 && blockIdx.x < 512) dn_df_wg_times[blockIdx.x * 2 + (i_)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define DF_WG(i_) do {} while (0)
#endif

// ---------------------------------------------------------------------------------------------------------------------------------
// The back-projection as a launch of its own (the shipped form of the diffusion operator: projection and spectral step stay the split-V
// kernel + per-mesh reduce of dn_tngemm.hip / dn_pointwise.hip): out[rows] = Phi[rows] ys[mesh] (+ the backward's add + mass * acc) with
// the direct row product.  One 512-thread workgroup per CU owns the contiguous rows its plan entry names; the spectrum planes of its mesh
// are split once into LDS (96 KiB), Phi fragments come straight from memory -- the rows the projection kernel streamed two launches
// earlier: Infinity-Cache hits.  A kernel of its own rather than the third phase of a fused one: the register allocator sizes a
// kernel for its worst phase and spills in the hottest one -- the unit loop ran 68k cycles inside the archived one-launch kernel (27-51
// spilled registers, every reload behind a vmcnt(0) that drains the operand prefetch) against 38k when it is alone.
// ---------------------------------------------------------------------------------------------------------------------------------
struct BpArgs {
    const DnTile* plan; int n_wg;
    const float* evecs; const float* ys; float* out; const float* add; const float* rowv; float* out_amax;
    DnAmax a_amax, b_amax;       // NP = 2 (split-fp16 engine): magnitude bounds of Phi and of the spectrum (power-of-two operand scales)
};
// NP = 3: 3-term split-bf16 (the forward: its output is what the gradient operators difference); NP = 2: 2-term split-fp16 with
// power-of-two operand scales from the producers' magnitude words (the backward of the fused block, as in rounds 3-4): half the MFMAs,
// 6 instead of 11 split instructions per operand pair, 64 instead of 96 KiB of planes.
template <int MODE, int NP>
__global__ __launch_bounds__(DN_TX_THREADS) DN_WAVES_PER_EU(2) void backproject_kernel(BpArgs a) {
    constexpr int K = 128, C = 128;
    DN_DYN_SMEM(smem_raw);
    unsigned char* smem = reinterpret_cast<unsigned char*>(smem_raw);
    float* swmax = reinterpret_cast<float*>(smem + DN_RD_LDS_B);
    const int tid = threadIdx.x, lane = tid & 63, wave = DN_UNIFORM(tid >> 6);
    const DnTile me = a.plan[blockIdx.x];
    float om = 0.f;
    float sa = 1.f, sb = 1.f, so = 1.f;
    if constexpr (NP == 2) {
        sa = dn_pow2_scale(dn_amax_eval(a.a_amax));
        sb = dn_pow2_scale(dn_amax_eval(a.b_amax));
        so = (1.f / sa) * (1.f / sb);
    }
    DF_WG(0);
    if (me.mesh >= 0 && me.nrows > 0) {
        // the wave's first two 16-row units of Phi are requested BEFORE the planes are staged (they do not depend on them): 98.3 vs 100.1 us
        // for the forward operator, 115.7 vs 116.7 backward (profiles/r05_backproject_ab.txt; streaming stores / loads measured too: slower)
        RdStart st;
        rd_rows_begin(a.evecs, K, me.row0, me.row0 + me.nrows, wave, lane, st);
        rd_stage_b_nn<DN_TX_THREADS, NP>(a.ys + (long long)me.mesh * K * C, C, smem, tid, sb);
        __syncthreads();
        RgArgs rg;
        rg.o0 = a.out; rg.ldo = C; rg.ldr = C; rg.N = C; rg.r0 = a.add; rg.rowv = a.rowv; rg.bias = nullptr; rg.mask = nullptr; rg.rng_seed = 0ull;
        rg.scale = 1.f;
        om = rd_rows_run<MODE, NP>(rg, smem, a.evecs, K, me.row0, me.row0 + me.nrows, 0, lane, st, sa, so);
        __syncthreads();
        DF_WG(1);
    }
    if (a.out_amax) {      // one check-first atomic per workgroup
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) { const float o = __shfl_xor(om, d, 64); om = o > om ? o : om; }
        __syncthreads();
        if (lane == 0) swmax[wave] = om;
        __syncthreads();
        if (tid == 0) {
            float mm = 0.f;
            for (int w = 0; w < DN_TX_THREADS / 64; ++w) mm = swmax[w] > mm ? swmax[w] : mm;
            if (mm > 0.f && mm > *reinterpret_cast<volatile float*>(a.out_amax)) atomicMax(reinterpret_cast<unsigned*>(a.out_amax), __float_as_uint(mm));
        }
    }
}
template <int MODE, int NP>
static int bp_launch(const BpArgs& a, hipStream_t stream) {
    const size_t smem = (size_t)DN_RD_LDS_B + 64;
#ifndef DN_EMULATE
    static unsigned long long lds_opt_in = 0;
    { const int oe_ = dn_lds_opt_in(reinterpret_cast<const void*>(&backproject_kernel<MODE, NP>), smem, &lds_opt_in); if (oe_) return oe_; }
#endif
    DN_LAUNCH((backproject_kernel<MODE, NP>), dim3(a.n_wg, 1, 1), dim3(DN_TX_THREADS, 1, 1), smem, stream, a);
    return (int)hipGetLastError();
}
// out = evecs ys (mass == null) or add + mass * (evecs ys); plan: dn_diffuse_plan_host()
// f16: run on the split-fp16 engine with operand magnitudes a_amax (Phi) / b_amax (the spectrum)
int dn_launch_backproject(const DnTile* plan, int n_wg, const float* evecs, const float* ys, float* out, const float* add, const float* mass,
                          float* out_amax, double acct_rows, hipStream_t stream, int f16, const DnAmax* a_amax, const DnAmax* b_amax) {
    if (!plan || n_wg <= 0 || (f16 && (!a_amax || !b_amax))) return DN_ERR_BAD_MODE;
    BpArgs a;
    memset(&a, 0, sizeof(a));
    a.plan = plan; a.n_wg = n_wg; a.evecs = evecs; a.ys = ys; a.out = out; a.add = add; a.rowv = mass; a.out_amax = out_amax;
    if (f16) { a.a_amax = *a_amax; a.b_amax = *b_amax; }
    dn_prof_begin(DN_K_BACKPROJECT, stream);
    const int err = f16 ? (mass ? bp_launch<DN_EPI_MASS_ADD, 2>(a, stream) : bp_launch<DN_EPI_STORE, 2>(a, stream))
                        : (mass ? bp_launch<DN_EPI_MASS_ADD, 3>(a, stream) : bp_launch<DN_EPI_STORE, 3>(a, stream));
    dn_prof_end(DN_K_BACKPROJECT, stream, 2.0 * acct_rows * 128 * 128, 4.0 * acct_rows * ((mass ? (add ? 3 : 2) : 2) * 128.0 + (mass ? 1 : 0)));
    return err;
}

// ---- the plan: which rows of which mesh every workgroup owns (host arithmetic; the caller uploads it)
// sizes: vertices per mesh (row order).  plan: [n_wg] entries {row0, nrows, mesh, aux = first_slot_of_mesh * 1024 + n_slots_of_mesh}, mesh < 0:
// idle; returns 1, or 0: this batch is not taken (more meshes than workgroups, an empty mesh).
int dn_diffuse_plan_host(const int* sizes, int n_mesh, int n_wg, DnTile* plan) {
    if (n_mesh <= 0 || n_wg <= 0) return 0;
    long long V = 0;
    for (int m = 0; m < n_mesh; ++m) { if (sizes[m] <= 0) return 0; V += sizes[m]; }
    if (n_mesh > n_wg || n_mesh > 4096) return 0;
    // workgroups per mesh: proportional to its rows, at least 1, at most 128 and rows / 64 (the caps the plan has had since round 5)
    int cnt[4096], cap[4096];
    int sum = 0;
    for (int i = 0; i < n_mesh; ++i) {
        const int v = sizes[i];
        cap[i] = v / 64 < 1 ? 1 : (v / 64 > 128 ? 128 : v / 64);
        long long q = (long long)n_wg * v / V;
        cnt[i] = q < 1 ? 1 : (q > cap[i] ? cap[i] : (int)q);
        sum += cnt[i];
    }
    while (sum > n_wg) {                                           // (only when many tiny meshes forced the minimum of one)
        int big = 0;
        for (int i = 1; i < n_mesh; ++i) if (cnt[i] > cnt[big]) big = i;
        if (cnt[big] <= 1) return 0;
        --cnt[big]; --sum;
    }
    bool prog = true;
    while (sum < n_wg && prog) {                                   // remainder to the meshes with the most rows per workgroup
        prog = false;
        int best = -1;
        double bestv = 0.0;
        for (int i = 0; i < n_mesh; ++i)
            if (cnt[i] < cap[i]) { const double r = (double)sizes[i] / cnt[i]; if (r > bestv) { bestv = r; best = i; } }
        if (best >= 0) { ++cnt[best]; ++sum; prog = true; }
    }
    long long row0 = 0;
    int slot = 0;
    for (int i = 0; i < n_mesh; ++i) {
        const int v = sizes[i], c = cnt[i], first = slot;
        int prev = 0;
        for (int j = 0; j < c; ++j) {
            int end = (j == c - 1) ? v : (int)(((long long)v * (j + 1) / c + 8) / 16 * 16);
            if (end <= prev) end = prev + 1;
            if (end > v - (c - 1 - j)) end = v - (c - 1 - j);
            DnTile t;
            t.row0 = (int)(row0 + prev); t.nrows = end - prev; t.mesh = i; t.aux = first * 1024 + c;
            plan[slot++] = t;
            prev = end;
        }
        row0 += v;
    }
    for (; slot < n_wg; ++slot) { DnTile t; t.row0 = 0; t.nrows = 0; t.mesh = -1; t.aux = 0; plan[slot] = t; }
    return 1;
}
