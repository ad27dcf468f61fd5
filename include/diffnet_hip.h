/* diffnet_hip.h -- C ABI of libdiffnet_hip.so: the MI355X (gfx950) DiffusionNet hot path.
 *
 * The reference (nmwsharp/diffusion-net) has no native layer: its hot path is Python calling
 * stock ATen kernels.  This header is the boundary a maintainer binds instead (ctypes stub in
 * INTEGRATION.md).  Every entry point cites the reference interface it replaces
 * (file:line under src/diffusion_net/).
 *
 * Conventions (all entry points):
 *   - return value: hipError_t as int, 0 = success; never throws;
 *   - never allocates, frees or synchronises; all work is enqueued on `stream` (a hipStream_t);
 *   - every pointer inside dn_mesh_batch_t / dn_block_* and every float* / int* argument is a
 *     DEVICE pointer owned by the caller and kept alive until the stream has drained; the structs
 *     themselves live in host memory and are read during the call only;
 *   - dense arrays are row-major contiguous fp32; index arrays int32; masks uint8 (1 = keep);
 *   - `ws` is caller-provided device scratch of at least the size the matching
 *     dn_*_workspace_bytes() reports; contents are undefined on return;
 *   - re-entrant: the compute path reads no environment variables and writes no global state.  Three process-wide pieces of
 *     bookkeeping exist: the opt-in timing of dn_prof_* (off by default), a per-device "large-LDS attribute set" bitmap per kernel
 *     instantiation (set-once, idempotent), and the table of tuning options behind dn_set_option() (kernel selection for A/B runs and
 *     tests; relaxed atomics written only by that call, read by the entry points at call time -- a value must not change between a
 *     *_workspace_bytes() query and the call it sizes, nor between the warm-up and the capture of a HIP graph; per-call engine choices
 *     go through dn_block_params_t.flags instead);
 *   - every struct below must be ZERO-INITIALISED by the caller before its fields are filled (memset): fields are only ever appended, and
 *     an appended field's zero value selects the behaviour of the versions before it.  dn_version() identifies the layout generation.
 *
 * A "mesh batch" is a ragged batch of independent meshes whose vertex axes are concatenated:
 * mesh m owns rows [mesh_rows[m].row0, +nrows) of every [v_total, *] array; the sparse gradient
 * operators use global (concatenated) row/column indices, i.e. they are block-diagonal.
 * Table invariants: meshes, tiles and chunks are listed in row order and each table covers [0, v_total) without gaps or
 * overlap; a tile / chunk never straddles two meshes.
 */
#ifndef DIFFNET_HIP_H
#define DIFFNET_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DN_MAX_MLP_LAYERS 8

/* a run of rows that belongs to one mesh (tiles: <= dn_tile_rows() rows; chunks: any length) */
typedef struct { int32_t row0, nrows, mesh, aux; } dn_tile_t;

/* Per-batch geometry: what geometry.get_operators() returns per mesh (geometry.py:426-570),
 * packed for the device.  gradX/gradY share one CSR pattern (geometry.py:381-382). */
typedef struct dn_mesh_batch {
    int32_t n_mesh, v_total, k_eig, n_tiles, n_chunks, g_nnz;  /* g_nnz: non-zeros of the gradient pattern */
    const dn_tile_t* tiles;          /* [n_tiles]  row tiles of <= dn_tile_rows() rows              */
    const dn_tile_t* chunks;         /* [n_chunks] split-V chunks, grouped by mesh                   */
    const int32_t*   mesh_chunk_off; /* [n_mesh+1] chunk range of every mesh                         */
    const dn_tile_t* mesh_rows;      /* [n_mesh]   {row0, nrows, m, 0}                               */
    const float* mass;               /* [v_total]            lumped vertex areas                     */
    const float* evals;              /* [n_mesh, k_eig]      Laplacian eigenvalues                   */
    const float* evecs;              /* [v_total, k_eig]     mass-orthonormal eigenbasis             */
    const int32_t* g_rowptr;  const int32_t* g_col;  const float* g_vx;  const float* g_vy;   /* CSR of gradX/gradY  */
    const int32_t* gt_rowptr; const int32_t* gt_col; const float* gt_vx; const float* gt_vy;  /* CSR of transposes   */
    /* Optional (round 3): one device float each holding max |evecs| and max |mass| (any upper bound within ~2^10 is as good) -- the
     * operand magnitudes the split-fp16 matrix engine of the fused block scales by.  NULL: the block calls measure them themselves
     * (one extra pass over the eigenbasis per call). */
    const float* evecs_amax; const float* mass_amax;
    /* Optional: one device float holding the infinity norm of the stacked gradient operators, max_i sum_j max(|gradX_ij|, |gradY_ij|)
     * summed as sum_j |gradX_ij| resp. sum_j |gradY_ij| (the larger of the two row sums): max |gradX x|, |gradY x| <= it * max |x| is
     * the magnitude bound the split-fp16 gradient-feature products scale by (about 3x the true maximum on a mesh).  NULL: measured. */
    const float* grad_norm;
    /* Optional (round 5): the work plan of the diffusion's direct back-projection launch (dn_diffusion_plan()): device array of df_n_wg
     * entries; df_n_groups is 1 when a plan is attached.  NULL / 0: the back-projection is the row GEMM. */
    const dn_tile_t* df_plan; int32_t df_n_wg, df_n_groups;
    /* Optional (round 6): the spectral-gradient operands of the batch (dn_spectral_pack_f32): the spatial gradient apply re-associated
     * through the eigenbasis, gradX (evecs ys) = (gradX evecs) ys.  sg_pack: [evecs | gradX evecs | gradY evecs] as fp16 (hi, lo) operand
     * fragments, 16 rows per group, every mesh padded to whole units of 64 (k_eig <= 128) / 128 (k_eig = 256) rows; sg_units: [sg_n_units] the units ({row0, nrows, mesh, 0},
     * dn_spectral_units()); sg_amax: [n_mesh][4] floats, the per-mesh magnitudes the fragments were scaled by.  With them the block forward
     * computes xd, gx, gy inside its chained row kernel (no back-projection launch, no CSR gather) for the shapes
     * dn_spectral_grad_supported() names.  NULL / 0: back-projection + gather, as before. */
    const void* sg_pack; const dn_tile_t* sg_units; const float* sg_amax; int32_t sg_n_units;
    /* Stamp of df_plan (round 6): v_total of the batch dn_diffusion_plan() was called for.  The plan names rows the kernels write: a plan whose
     * stamp is not this batch's v_total, or whose df_n_wg is not dn_diffusion_plan_wgs() of the current device, is IGNORED (row GEMM instead) --
     * a caller that leaves the field zero therefore never takes the planned kernels. */
    int32_t df_v_total;
} dn_mesh_batch_t;

/* Weights of one DiffusionNetBlock (layers.py:167-198), nn.Linear layout: W[out][in]. */
typedef struct dn_block_params {
    int32_t C, n_mlp, with_grad, with_rot;
    int32_t widths[DN_MAX_MLP_LAYERS + 1]; /* MiniMLP sizes: widths[0] = 3C (2C w/o gradient features), ..., widths[n_mlp] = C */
    const float* time;                     /* [C] diffusion_time, clamped to >= 1e-8 (layers.py:48-49) -- by the caller, or see clamp_time */
    const float* A_re; const float* A_im;  /* [C,C] (with_rot=0: A_re holds A, A_im ignored), layers.py:110-113 */
    const float* W[DN_MAX_MLP_LAYERS];     /* [widths[i+1], widths[i]] */
    const float* b[DN_MAX_MLP_LAYERS];     /* [widths[i+1]] */
    const uint8_t* mask[DN_MAX_MLP_LAYERS];/* mask[i], i>=1: dropout keep-mask of layer i's INPUT [v_total, widths[i]]
                                              (layers.py:143-147), NULL = no mask given; kept values are scaled by 2 */
    uint64_t drop_seed;                    /* != 0 and mask[i] == NULL: nn.Dropout(p=.5) of layer i's input is drawn IN the
                                              producing kernel's epilogue, keep = bit of hash(drop_seed, i, row, column): no mask
                                              tensor is written or read (the backward needs none: a saved activation is > 0
                                              exactly where it was kept and active).  0 = no dropout where mask[i] == NULL. */
    const uint64_t* drop_seed_dev;         /* optional DEVICE word added to drop_seed inside the kernels: a captured HIP graph of the training
                                              step advances it with a graph node, so that every replay draws new masks without host work */
    /* Optional (round 3), magnitudes for the split-fp16 engine: x_amax = device float holding max |x| of the block input (the previous
     * block's out_amax); NULL: measured by the call (one extra pass over x).  out_amax: device float that receives max |out| (zeroed by
     * the call when dn_block_tracks_amax() says the call tracks magnitudes, untouched otherwise), or NULL. */
    const float* x_amax; float* out_amax;
    /* Optional (round 4): != 0 makes dn_block_fwd_f32 raise `time` to >= 1e-8 IN PLACE before anything reads it -- the clamp the reference
     * applies to the parameter in every forward (layers.py:48-49: the Parameter keeps the clamped values) -- as part of the call's first
     * launch, instead of a separate elementwise kernel of the caller.  `time` must then be writable.  The backward ignores the field. */
    int32_t clamp_time;
    /* Optional (round 6): per-call engine choice, overriding the process-wide dn_set_option() table for THIS call (two models in one process may
     * want different engines; the table is for A/B runs).  0 = follow the table.  Workspace queries take the same params, so a call and its
     * query always agree. */
    uint32_t flags;
} dn_block_params_t;
#define DN_BLOCK_NO_CHAIN 1u                 /* unfused launches instead of the chained row kernels                  */
#define DN_BLOCK_NO_F16 2u                   /* split-bf16 engine throughout (implies the unfused launches)          */
#define DN_BLOCK_NO_SPECTRAL_GRAD 4u         /* back-projection + CSR gather even if the batch carries sg_pack       */
#define DN_BLOCK_SPECTRAL_GRAD_ALWAYS 8u     /* spectral-gradient forward at every size (option "spectral_grad" = 2) */

/* Activations the forward saves for the backward (caller-allocated). */
typedef struct dn_block_saved {
    float* xs;                         /* [n_mesh, k_eig, C]  spectrum of x                     */
    float* xd;                         /* [v_total, C]        diffused features                 */
    float* gx; float* gy;              /* [v_total, C]        spatial gradients   (with_grad)   */
    float* g; float* bre; float* bim;  /* [v_total, C]        tanh features, rotated gradients  */
    float* h[DN_MAX_MLP_LAYERS];       /* h[i], i < n_mlp-1: [v_total, widths[i+1]] post-ReLU(+dropout) */
    float* amax;                       /* optional [DN_BLOCK_AMAX_WORDS] device floats: magnitudes of the saved activations (written by the
                                          forward, read by the backward).  NULL: both calls use the split-bf16 engine throughout. */
    /* Optional (round 7): the signs of the hidden activations as bit words, one array per hidden layer i < n_mlp-1 whose width is C, for
     * C = 64 and C = 128 (no words exist at other widths: the field is ignored there).  hbits[i]: [v_total][4] uint32, 16 bytes per row; the word
     * at (row, q) has bit 4 nt + e set iff h[i][row][16 nt + 4 q + e] > 0 (C = 128: all 32 bits, C = 64: the low 16; the other bits are zero).
     * A non-NULL hbits[i] is WRITTEN by dn_block_fwd_f32 on every route (by the chained row kernel from the values it stores, else by one small
     * pass over the stored h[i]) and READ by dn_block_bwd_f32 whenever its chained row kernel runs, which then does not read h[i] (the
     * weight-gradient products still do: h stays in the saved set).  All of hbits[i], i < n_mlp-1, or none: NULL = the behaviour of version 600
     * in both directions.  Results are bit-identical either way (the same predicate on the same fp32 value). */
    uint32_t* hbits[DN_MAX_MLP_LAYERS];
} dn_block_saved_t;
#define DN_BLOCK_AMAX_WORDS 16

typedef struct dn_block_grads {
    float* d_x;                        /* [v_total, C] */
    float* d_time;                     /* [C] */
    float* dA_re; float* dA_im;        /* [C,C] (with_rot=0: dA_re holds dA) */
    float* dW[DN_MAX_MLP_LAYERS];
    float* db[DN_MAX_MLP_LAYERS];
    const float* d_out_amax;           /* optional: device float with max |d_out| (the next block's d_x_amax); NULL: measured by the call */
    float* d_x_amax;                   /* optional: device float that receives max |d_x| */
} dn_block_grads_t;

int dn_version(void);         /* 700: dn_block_saved_t.hbits; 600: round-6 layout (dn_mesh_batch_t.sg_pack ...); 500: round 5 (dn_mesh_batch_t.df_plan ..., dn_set_option) */
int dn_tile_rows(void);      /* rows per entry of dn_mesh_batch_t.tiles (128) */
int dn_tn_target_chunks(void);  /* how many entries dn_mesh_batch_t.chunks should have on the current device for the split-V products to fill it in
                                   whole rounds: one workgroup slot per CU (wave-specialised kernel).  Any chunk list is CORRECT; this one is fastest. */
int dn_tn_target_chunks_k(int k_eig);   /* (round 6) the same for a batch of k_eig eigenvectors per mesh: from k_eig = 256 on half as many chunks -- every chunk
                                   writes a k_eig x C partial that the spectral step reads back (one 200k-vertex mesh, K = C = 256: projection 210 -> 190 us,
                                   block inference 1388 -> 1347 us with 240 instead of 489 chunks; profiles/r06_chunks256.txt) */

/* ---- tuning options (no reference counterpart): process-wide integers the entry points read at call time, for A/B measurements and for
 *      tests that must run a particular kernel.  Unknown names return non-zero.  Defaults in parentheses.
 *        "chain" (1)            chained row kernels of the fused block (0: unfused launches)
 *        "chain_min_rows" (0)   smallest batch the TRAINING forward takes the chained kernel for ...
 *        "chain_small_rows" (0)      ... and the largest small batch below that which takes it all the same (a window for the unfused launches: tests)
 *        "chain_hh" (0)         16-row halves per wave of the chained kernels (0: by batch size and direction, dn_api.hip; the forward
 *                               kernel of C = 256 has one shape -- two halves, four waves -- and ignores this option and the next)
 *        "chain_nw" (0)         waves per workgroup of the chained kernels (0: chosen by batch size)
 *        "f16" (1)              split-fp16 matrix engine for the row products of the fused block (0: split-bf16 everywhere)
 *        "f16_mask" (188)       product classes on the split-fp16 engine (diagnostic bit mask, dn_api.hip)
 *        "f16_wgrad" (0)        parameter-gradient products on the split-fp16 engine (diagnostic)
 *        "diffuse" (2)          batches that carry a plan (dn_diffusion_plan), K = C = 128: non-zero = the back-projection of the diffusion is the
 *                               direct row-product launch (dn_diffuse.hip: backproject_kernel); 0 = the wave-specialised row GEMM of the earlier rounds
 *        "spectral_grad" (1)    batches that carry spectral-gradient operands (dn_spectral_pack_f32): the chained forward kernel computes xd, gx, gy
 *                               from them (no back-projection launch, no CSR gather) -- 1 = in the inference forward at every size and in the training
 *                               forward up to 65536 rows, both at C <= 128 (where it measures faster), 2 = wherever a form exists (incl. the two-launch
 *                               form of k_eig = C = 256, which measures slower), 0 = never (back-projection + gather) */
int dn_set_option(const char* name, int value);
int dn_get_option(const char* name, int* value);

/* ---- opt-in per-kernel timing for benchmarks (no reference counterpart; the one piece of mutable global
 *      state, off by default): every launch is bracketed by hipEvents on its stream and summed per kernel
 *      kernel kind in [0, 11) (dn_prof_kind_name(kind) is "" past the last one).  read: out[0..3] = {ms, launches, algorithmic flops, algorithmic bytes}. */
int dn_prof_enable(int on);
int dn_prof_reset(void);
int dn_prof_read(int kind, double* out);
const char* dn_prof_kind_name(int kind);

/* ---- geometry.to_basis (geometry.py:572-583): spec[m] = evecs_m^T (x_m * mass_m); use_mass=0 drops the mass
 *      (the autograd transpose of from_basis).  spec: [n_mesh, k_eig, C]. */
size_t dn_to_basis_workspace_bytes(const dn_mesh_batch_t* mb, int C);
int dn_to_basis_f32(const dn_mesh_batch_t* mb, const float* x, int C, int use_mass, float* spec,
                    void* ws, size_t ws_bytes, void* stream);
/* ---- geometry.from_basis (geometry.py:586-598): out_m = evecs_m spec[m].  out: [v_total, C].
 *      scale_rows_by_mass=1 multiplies row v by mass[v] (the autograd transpose of to_basis). */
int dn_from_basis_f32(const dn_mesh_batch_t* mb, const float* spec, int C, int scale_rows_by_mass, float* out, void* stream);

/* ---- LearnedTimeDiffusion.forward, method='spectral' (layers.py:44-67) and its gradient.
 *      fwd: xs = to_basis(x), xd = from_basis(exp(-evals*time) * xs).
 *      bwd: d_x = d_x_add + mass * (evecs (coef * evecs^T d_xd)), d_time[c] = -sum lambda*coef*xs*(evecs^T d_xd). */
/*      dn_diffuse.hip (direct back-projection launch): taken when mb->df_plan is set, k_eig = C = 128 and every operand is
 *      16-byte aligned (option "diffuse").
 *      dn_diffusion_plan_wgs(): workgroups the plan should be made for on the current device (one per CU).
 *      dn_diffusion_plan(): HOST arithmetic -- sizes[n_mesh] = vertices per mesh in row order; n_groups: reserved, pass 0 (ignored);
 *      plan: HOST array of DN_DIFFUSION_MAX_GROUPS * n_wg entries; returns 1, or 0: batch not plannable, leave df_plan NULL.  The
 *      caller uploads plan[0 .. n_wg) and sets df_plan, df_n_wg, df_n_groups = 1 and df_v_total. */
#define DN_DIFFUSION_MAX_GROUPS 1
int dn_diffusion_plan_wgs(void);
int dn_diffusion_plan(const int32_t* sizes, int n_mesh, int n_wg, int n_groups, dn_tile_t* plan);
size_t dn_diffusion_workspace_bytes(const dn_mesh_batch_t* mb, int C);
int dn_diffusion_fwd_f32(const dn_mesh_batch_t* mb, const float* x, const float* time, int C,
                         float* xs, float* xd, void* ws, size_t ws_bytes, void* stream);
int dn_diffusion_bwd_f32(const dn_mesh_batch_t* mb, const float* d_xd, const float* xs, const float* time, int C,
                         const float* d_x_add, float* d_x, float* d_time, void* ws, size_t ws_bytes, void* stream);

/* ---- spectral-gradient operands (dn_spectral.hip; no reference counterpart: layers.py:213-223 applies gradX / gradY to x_diffuse = evecs ys,
 *      which lies in the span of evecs -- gradX x_diffuse = (gradX evecs) ys exactly).  Built ONCE per mesh batch:
 *      dn_spectral_grad_supported(k_eig, C): 1 if the block forward takes the operands at this shape (k_eig = 128 with C in {64, 128};
 *      k_eig = C = 256).
 *      dn_spectral_units(): HOST arithmetic -- sizes[n_mesh] = vertices per mesh in row order -> units[] (NULL: count only) of <= 64 rows
 *      (k_eig <= 128) or <= 128 rows (k_eig = 256) of one mesh each; returns the count.
 *      dn_spectral_pack_bytes(n_units, k_eig): bytes of the packed operand.  dn_spectral_pack_workspace_bytes(): scratch of the pack call.
 *      dn_spectral_pack_f32(): mb needs evecs, the gradient CSR and k_eig % 32 == 0; units = DEVICE copy of the unit table; writes
 *      sg_pack[dn_spectral_pack_bytes] and sg_amax[4 n_mesh]; gradX evecs / gradY evecs are accumulated in fp64 in entry order (deterministic).
 *      The caller then sets mb->sg_pack / sg_units / sg_amax / sg_n_units. */
int dn_spectral_grad_supported(int k_eig, int C);
int dn_spectral_units(const int32_t* sizes, int n_mesh, int k_eig, dn_tile_t* units);
size_t dn_spectral_pack_bytes(int n_units, int k_eig);
size_t dn_spectral_pack_workspace_bytes(const dn_mesh_batch_t* mb);
int dn_spectral_pack_f32(const dn_mesh_batch_t* mb, const dn_tile_t* units, int n_units, void* sg_pack, float* sg_amax,
                         void* ws, size_t ws_bytes, void* stream);

/* ---- spatial gradient apply, layers.py:217-223 (gx = gradX x, gy = gradY x) and its transpose
 *      d_x = add + gradX^T d_gx + gradY^T d_gy (add may be NULL). */
int dn_grad_apply_fwd_f32(const dn_mesh_batch_t* mb, const float* x, int C, float* gx, float* gy, void* stream);
int dn_grad_apply_bwd_f32(const dn_mesh_batch_t* mb, const float* d_gx, const float* d_gy, const float* add, int C,
                          float* d_x, void* stream);

/* ---- SpatialGradientFeatures.forward (layers.py:117-130): g = tanh(gx*Bre + gy*Bim).
 *      A_im = NULL selects with_gradient_rotations=False (layers.py:125-126).  bre/bim may be NULL (inference). */
size_t dn_gradfeat_workspace_bytes(const dn_mesh_batch_t* mb, int C);
int dn_gradfeat_fwd_f32(const dn_mesh_batch_t* mb, const float* gx, const float* gy, const float* A_re, const float* A_im,
                        int C, float* g, float* bre, float* bim, void* stream);
int dn_gradfeat_bwd_f32(const dn_mesh_batch_t* mb, const float* d_g, const float* g, const float* gx, const float* gy,
                        const float* bre, const float* bim, const float* A_re, const float* A_im, int C,
                        float* d_gx, float* d_gy, float* dA_re, float* dA_im, void* ws, size_t ws_bytes, void* stream);

/* ---- nn.Linear (first_lin / last_lin, layers.py:297-298,366,373; MiniMLP layers, layers.py:150-164):
 *      out = act(x W^T + b) [* 2*mask];  relu/mask as in MiniMLP.  bwd: d_x = d_out W (skipped when d_x NULL),
 *      dW = d_out^T x, db = column sums of d_out. */
size_t dn_linear_workspace_bytes(const dn_mesh_batch_t* mb, int C_in, int C_out);
int dn_linear_fwd_f32(const dn_mesh_batch_t* mb, const float* x, int C_in, const float* W, const float* b, int C_out,
                      int relu, const uint8_t* mask, float* out, void* stream);
int dn_linear_bwd_f32(const dn_mesh_batch_t* mb, const float* d_out, const float* x, const float* W, int C_in, int C_out,
                      float* d_x, float* dW, float* db, void* ws, size_t ws_bytes, void* stream);
/* The same two products, additionally leaving max |out| (max |d_x|) in a device word for the split-fp16 engine of the block that
 * consumes the result (dn_block_params_t.x_amax / dn_block_grads_t.d_out_amax): first_lin feeds block 0, last_lin's input gradient feeds
 * the last block's backward.  The word is ACCUMULATED into (atomic max): the caller zeroes it.  NULL = not tracked (the plain forms).
 * Thin products (C_in <= 16 forward, C_out <= 16 backward) track inside their kernel; others take one measuring pass. */
int dn_linear_fwd_amax_f32(const dn_mesh_batch_t* mb, const float* x, int C_in, const float* W, const float* b, int C_out,
                           int relu, const uint8_t* mask, float* out, float* out_amax, void* stream);
int dn_linear_bwd_amax_f32(const dn_mesh_batch_t* mb, const float* d_out, const float* x, const float* W, int C_in, int C_out,
                           float* d_x, float* dW, float* db, float* d_x_amax, void* ws, size_t ws_bytes, void* stream);

/* ---- DiffusionNetBlock.forward (layers.py:200-241) and its backward, fused orchestration.
 *      saved = NULL runs inference (intermediates live in ws). */
size_t dn_block_fwd_workspace_bytes(const dn_mesh_batch_t* mb, const dn_block_params_t* p, int with_saved);
/*      1 if the block call `call` (0: dn_block_fwd_f32 without saved activations, 1: dn_block_fwd_f32 with them, 2: dn_block_bwd_f32) on this batch
 *      and these parameters writes the optional magnitude words (out_amax and saved->amax / d_x_amax), 0 if it leaves them untouched (shapes
 *      neither the split-fp16 engine nor the chained kernels take): a caller that hands the words on to the next block must not hand on words
 *      nobody wrote. */
int dn_block_tracks_amax(const dn_mesh_batch_t* mb, const dn_block_params_t* p, int call);
size_t dn_block_bwd_workspace_bytes(const dn_mesh_batch_t* mb, const dn_block_params_t* p);
int dn_block_fwd_f32(const dn_mesh_batch_t* mb, const dn_block_params_t* p, const float* x, float* out,
                     const dn_block_saved_t* saved, void* ws, size_t ws_bytes, void* stream);
int dn_block_bwd_f32(const dn_mesh_batch_t* mb, const dn_block_params_t* p, const float* x,
                     const dn_block_saved_t* saved, const float* d_out, const dn_block_grads_t* grads,
                     void* ws, size_t ws_bytes, void* stream);

/* ---- operator packing: sparse COO (int64 indices, as the reference holds gradX/gradY: utils.py:55, geometry.py:375-382) -> int32 CSR of
 *      the pattern and CSR of its transpose, values carried along; also builds the gather patterns of the faces/edges remap.
 *      rows: [nnz] non-decreasing row ids (coalesced COO order), or NULL: entry j belongs to row j / row_div (a dense [n_rows, row_div]
 *      index array such as faces).  cols: [nnz].  vx / vy: [nnz] values on the shared pattern (either may be NULL).
 *      Out: rowptr [n_rows+1], col [nnz]; transpose: t_rowptr [n_cols+1], t_col [nnz] (row ids, ascending inside a transposed row),
 *      t_vx / t_vy [nnz].  status: one device int32, non-zero afterwards if an index was outside [0,n_rows) x [0,n_cols) or the
 *      rows were not sorted (the outputs are then undefined; the caller checks it at its next synchronisation point). */
size_t dn_coo_to_csr_workspace_bytes(int64_t nnz, int n_cols);
int dn_coo_to_csr_i64(const int64_t* rows, int row_div, const int64_t* cols, const float* vx, const float* vy, int64_t nnz, int n_rows,
                      int n_cols, int32_t* rowptr, int32_t* col, int32_t* t_rowptr, int32_t* t_col, float* t_vx, float* t_vy,
                      int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* ---- content checksum for the device-resident operator cache (the reference re-uploads the operators of a mesh every step,
 *      human_segmentation_original.py:111-120, and caches them on disk by a hash of the mesh, geometry.py:476-494: the device-side analogue).
 *      Adds a 128-bit, order-independent checksum of the nbytes at `data` (multiple of 4, 4-byte aligned) to acc[0..1] (device, zeroed by
 *      the caller).  `salt` separates operands that share one accumulator.  EVERY byte of the operand enters the sum. */
int dn_checksum128(const void* data, size_t nbytes, uint64_t salt, uint64_t* acc, void* stream);
/*      The same for up to 16 buffers in ONE launch: data / nbytes / salts are HOST arrays of n entries (device pointers, byte counts, salts).
 *      Gives exactly the sum the n single calls would. */
int dn_checksum128_multi(int n, const void* const* data, const size_t* nbytes, const uint64_t* salts, uint64_t* acc, void* stream);

/* ---- output remaps (layers.py:379-397).
 *      csr_mean: out[i] = (sum_{j in row i} x[col[j]]) / div  -- faces (div=3) / edges (div=2) gather-mean, and with the
 *      transposed pattern its gradient.  mass_mean: out[m] = sum_v mass*x / sum_v mass per mesh (global_mean). */
int dn_csr_mean_f32(const int32_t* rowptr, const int32_t* col, int n_rows, const float* x, int C, float div,
                    float* out, void* stream);
int dn_mass_mean_fwd_f32(const dn_mesh_batch_t* mb, const float* x, int C, float* out, float* mass_sum, void* stream);
int dn_mass_mean_bwd_f32(const dn_mesh_batch_t* mb, const float* mass_sum, const float* d_out, int C, float* d_x,
                         void* stream);

/* ---- the head on the far side of the path, one pass each way (dn_head.hip): [gather-mean of the 2/3 vertices of an edge/face,
 *      layers.py:379-391] -> [log_softmax, the scripts' last_activation, human_segmentation_original.py:75] -> log-probabilities ->
 *      [NLL, F.nll_loss at human_segmentation_original.py:136 / rna_mesh_segmentation.py:135, or with smoothing > 0 the label-smoothed
 *      log loss of utils.py:18-24; mean over the rows whose label lies in [0, C) -- others (ignore_index) neither contribute nor count].
 *      Every bracketed stage is optional: rowptr = NULL: output i = row i (n_out == n_src); log_softmax = 0: x already holds
 *      log-probabilities; labels = NULL: no loss; logp = NULL: log-probabilities not written.  div: entries per output (3 faces, 2 edges).
 *      loss / count: device scalars (count = number of valid rows, needed by the backward).
 *      bwd: d_x[v] = sum_{i gathered v} (1/div) (dlp_i - [log_softmax] exp(logp_i) sum_c dlp_i[c]),
 *           dlp_i = d_logp_i (optional) - d_loss/count * smoothed-one-hot(label_i) (optional); t_rowptr/t_col: transposed gather. */
size_t dn_head_workspace_bytes(void);
int dn_head_fwd_f32(const float* x, int n_src, int C, const int32_t* rowptr, const int32_t* col, int n_out, float div, int log_softmax,
                    const int64_t* labels, float smoothing, float* logp, float* loss, float* count, void* ws, size_t ws_bytes, void* stream);
int dn_head_bwd_f32(const float* logp, int n_out, int C, const int32_t* t_rowptr, const int32_t* t_col, int n_src, float div, int log_softmax,
                    const int64_t* labels, float smoothing, const float* d_logp, const float* d_loss, const float* count, float* d_x,
                    void* stream);

/* ---- geometry.compute_hks (geometry.py:600-628; compute_hks_autoscale :630-633 passes scales = logspace(-2, 0, S)):
 *      out[b][v][s] = sum_k exp(-evals[b][k] * scales[.][s]) * evecs[b][v][k]^2.  evals [B,K], evecs [B,V,K], out [B,V,S];
 *      scales [S] shared by the batch (scales_per_batch = 0) or [B,S] (scales_per_batch = 1).  Forward only (an input feature). */
int dn_hks_f32(const float* evals, const float* evecs, const float* scales, int B, int V, int K, int S, int scales_per_batch,
               float* out, void* stream);

/* ---- geometry.find_knn (geometry.py:667-724): exact brute-force k-nearest-neighbour search that never forms the N x M matrix (dn_knn.hip).
 *      src [n_src, dim], tgt [n_tgt, dim] fp32 row-major; dist [n_src, k] fp32, idx [n_src, k] int64.  Row i holds the k targets with the
 *      smallest Euclidean distance to src[i] in increasing order (largest: the k largest, decreasing); omit_diagonal: target i is no
 *      candidate of row i (needs n_src == n_tgt).  Distances are the reference's difference form (fp32 chain of (a_d - b_d)^2 over d, one
 *      sqrtf); the order key is that squared distance and equal keys go to the lower target index, for `largest` as well.  The result is
 *      bit-identical from run to run and for every n_split.  Inputs are assumed finite.
 *      n_split: 0 = the library chooses how many contiguous target slices to search in parallel; >= 1 = that many (clamped to the
 *      number of 64-target tiles).  More than one slice needs the workspace (partial lists, merged by a second kernel).
 *      Returns 0 on success (n_src == 0: nothing is launched) and non-zero WITHOUT launching for k < 1, k > DN_KNN_MAX_K,
 *      k > n_tgt - (omit_diagonal ? 1 : 0), dim < 1, omit_diagonal with n_src != n_tgt, or a workspace smaller than the query says. */
#define DN_KNN_MAX_K 32
int dn_knn_max_k(void);
size_t dn_knn_workspace_bytes(int n_src, int n_tgt, int dim, int k, int n_split);
int dn_knn_f32(const float* src, int n_src, const float* tgt, int n_tgt, int dim, int k, int largest, int omit_diagonal, int n_split,
               float* dist, int64_t* idx, void* ws, size_t ws_bytes, void* stream);

/* ---- the same search for dim <= 3 over a dense grid of cells (dn_knn_grid.hip): work grows with n_src k instead of n_src n_tgt, and
 *      dist / idx are the bits dn_knn_f32 writes (same pair arithmetic, same order (squared distance, lower target index)) for every
 *      cells_per_axis and every cell_budget, from run to run.  There is no `largest`.
 *      The targets are binned into G = dn_knn_grid_cells(n_tgt, k, dim, cells_per_axis) cells per axis over their bounding cube
 *      (cells_per_axis: 0 = the library's choice from (n_tgt, k, dim), > 0 = that many, clamped to 256 / 4096 / 2^22 for dim 3 / 2 / 1).
 *      A call is two steps with the caller's sort between them; every operand stays on the device and nothing synchronises:
 *        box [2 dim] fp32: the per-axis minimum, then the per-axis maximum, of tgt (computed by the caller);
 *        dn_knn_grid_keys_f32 writes tgt_key [n_tgt] int32, the cell of every target, and src_key [n_src] (NULL: not wanted);
 *        the caller provides tgt_order / src_order [n_tgt] / [n_src] int64, the permutations of a STABLE ascending sort of the keys, and
 *        cell_start [G^dim + 1] int32, cell_start[c] = the number of targets whose key is below c;
 *        dn_knn_grid_search_f32 gathers the targets in that order into the workspace and searches: every query visits the cells around
 *        its own in shells of growing Chebyshev radius and stops when no unseen cell can hold a closer target.
 *      cell_budget: a query that has visited more than this many cells without stopping scans all targets instead (< 0: the library's
 *      value dn_knn_grid_cell_budget(); 0: every query scans).  info: NULL, or two int32 words the caller zeroed -- the largest shell
 *      radius any query reached and the number of queries that scanned.
 *      Non-finite coordinates give unspecified neighbours but no out-of-range access and no unbounded loop (an index read from
 *      tgt_order / src_order / cell_start is clamped into range).
 *      Both calls return 0 on success (n_src == 0: the search launches nothing) and non-zero WITHOUT launching for dim outside 1..3,
 *      k < 1, k > DN_KNN_MAX_K, a negative size or cells_per_axis, a NULL required pointer; the search also for
 *      k > n_tgt - (omit_diagonal ? 1 : 0), omit_diagonal with n_src != n_tgt, or a workspace smaller than the query says. */
int dn_knn_grid_cells(int n_tgt, int k, int dim, int cells_per_axis);
int dn_knn_grid_cell_budget(void);
size_t dn_knn_grid_workspace_bytes(int n_src, int n_tgt, int dim, int k, int cells_per_axis);
int dn_knn_grid_keys_f32(const float* src, int n_src, const float* tgt, int n_tgt, int dim, int k, int cells_per_axis, const float* box,
                         int32_t* src_key, int32_t* tgt_key, void* stream);
int dn_knn_grid_search_f32(const float* src, int n_src, const float* tgt, int n_tgt, int dim, int k, int omit_diagonal, int cells_per_axis,
                           int cell_budget, const float* box, const int64_t* src_order, const int64_t* tgt_order, const int32_t* cell_start,
                           float* dist, int64_t* idx, int32_t* info, void* ws, size_t ws_bytes, void* stream);

/* ---- geometry.farthest_point_sampling (geometry.py:727-751): farthest point sampling with the sample loop on the device (dn_fps.hip).
 *      pts [V, 3] fp32 row-major, already normalised: one cloud, or n_clouds clouds packed back to back with offsets [n_clouds + 1] int64
 *      ON THE DEVICE (cloud c is rows offsets[c] .. offsets[c+1] - 1).  order [n_clouds, n_sample] int64: rows of the packed array in the
 *      order chosen; radii [n_clouds, n_sample] fp32: the squared distance of each sample to the nearest earlier one at the moment it was
 *      chosen (+inf for the first; it never increases); min_dist2 [V] fp32 or NULL: the squared distance of every point to the nearest of
 *      the n_sample samples.  start [n_clouds] int64 on the device (rows of the packed array, clamped into their cloud) names the first
 *      sample of every cloud; NULL: the point of smallest |p|^2, the lowest index among equals.
 *      Squared distances are (dx*dx + dy*dy) + dz*dz in fp32 with every product and sum rounded on its own (no FMA); the next sample is the
 *      point of largest min_d, the lowest index among equals.  The result is bit-identical from run to run and for both routes.  Once
 *      every min_d is 0 (more samples than distinct points) the lowest index of the cloud is chosen again.  Inputs are assumed finite;
 *      non-finite coordinates cannot cause an out-of-range access (no address depends on a point's value).
 *      route: 0 = the library chooses (resident when max_points <= dn_fps_resident_max_points(), else stepped), 1 = resident (one
 *      workgroup per cloud, one launch), 2 = stepped (one launch per sample + 1, many workgroups per cloud; needs the workspace).
 *      min_points / max_points: the sizes of the smallest and the largest cloud (host values: the call never reads device memory).
 *      dn_fps_workspace_bytes: 0 for the resident route; for the stepped route it depends on n_clouds and max_points only (min_d is kept
 *      at a per-cloud stride the call can check; n_points_total <= 0 answers 0).
 *      Returns 0 on success (n_clouds == 0: nothing is launched) and non-zero WITHOUT launching for n_sample < 1, n_sample > min_points,
 *      max_points < min_points, route == 1 with max_points beyond the capacity, an unknown route, n_clouds < 0 (stepped: > 65535), or a
 *      workspace smaller than the query says. */
int dn_fps_resident_max_points(void);
size_t dn_fps_workspace_bytes(int64_t n_points_total, int n_clouds, int max_points, int n_sample, int route);
int dn_fps_f32(const float* pts, const int64_t* offsets, int n_clouds, int min_points, int max_points, int n_sample, const int64_t* start,
               int route, int64_t* order, float* radii, float* min_dist2, void* ws, size_t ws_bytes, void* stream);

/* ---- point-cloud frames and gradient stencils (geometry.py:92-99, 114-123, 151-206, 209-273 for a cloud): what the reference computes
 *      per point from the indices of its k nearest neighbours, in one pass (dn_cloud.hip).  pts [n,3] fp32; nbr [n,k] int64 as dn_knn_f32
 *      writes them (omit_diagonal).  With e_j = pts[nbr[i,j]] - pts[i] (centred on the point, not on the neighbourhood mean):
 *        normal  the unit eigenvector of sum_j e_j e_j^T for its smallest eigenvalue (= the last right singular vector of the k x 3 matrix
 *                of the e_j).  The reference's sign is whatever LAPACK returns; here the component of largest magnitude is positive, equal
 *                magnitudes going to the lower axis.  Rank-deficient neighbourhoods (collinear, coincident) give a finite unit vector.
 *                normals_in != NULL: those [n,3] normals are used as they are, the estimate is skipped and `normals` is a copy.
 *        frame   rows basisX, basisY, normal: basisX = c - n (n.c) with c = e_x where |n_x| < 0.9, else e_y, divided by (|basisX| + 1e-6)
 *                (the reference's normalize(): deliberately not quite unit); basisY = n x basisX.
 *        row i   of the complex gradient operator, real part in g_vx, imaginary part in g_vy: with t_j = (e_j.basisX, e_j.basisY) and
 *                G = sum_j t_j t_j^T + 1e-5 I the coefficient of neighbour j is G^-1 t_j and that of i itself -sum_j G^-1 t_j.  Every row
 *                has k + 1 entries, g_rowptr[i] = i (k + 1): entry 0 is column i, entries 1..k the neighbours in nbr order.  A neighbour
 *                equal to i (the reference drops tail == tip edges) contributes nothing: its slot carries column i and the value 0, so
 *                summing equal columns of a row reproduces the reference.
 *      Inputs and outputs are fp32; everything from the coordinate differences on is fp64, rounded once at the store; the result is
 *      bit-identical from run to run.  status: one device int32, set to the number of rows that held an index outside [0,n); such a row
 *      reads nothing through it and writes zeros (normal, frame, columns, values; its g_rowptr entry stays i (k + 1)).  The caller reads the
 *      word at its next synchronisation point.
 *      Returns 0 on success (n == 0: nothing is launched) and non-zero WITHOUT launching for k < 1, k > DN_KNN_MAX_K, n < 0,
 *      n (k + 1) > INT32_MAX, or a NULL pointer other than normals_in while n > 0. */
int dn_cloud_operators_f32(const float* pts, int n, const int64_t* nbr, int k, const float* normals_in, float* normals, float* frames,
                           int32_t* g_rowptr, int32_t* g_col, float* g_vx, float* g_vy, int32_t* status, void* stream);

/* ---- point-cloud Laplacian and lumped mass from local Delaunay stars (dn_cloud_lap.hip): the construction of Sharp & Crane 2020, section
 *      5.7, WITHOUT the intrinsic / tufted re-triangulation that robust_laplacian applies to the triangles (the reference takes its
 *      point-cloud Laplacian from that package; this is not its arithmetic).  pts [n,3] fp32; nbr [n,k] int64 as dn_knn_f32 writes them
 *      (omit_diagonal); frames [n,3,3] fp32 as dn_cloud_operators_f32 writes them (rows basisX, basisY; the normal row is not read).
 *        star    With e_a = pts[nbr[i,a]] - pts[i], X_a = e_a.basisX, Y_a = e_a.basisY, W_a = X_a^2 + Y_a^2: the unordered pair {a, b} is a
 *                triangle of point i iff cr = X_a Y_b - Y_a X_b satisfies |cr| > 1e-12 sqrt(W_a W_b) and no other slot c lies strictly
 *                inside the circle through 0, a, b -- for cr > 0: W_c cr - W_b (X_a Y_c - Y_a X_c) + W_a (X_b Y_c - Y_b X_c) < 0.  A slot
 *                whose index is i itself or whose W is 0 takes no part, as vertex or as obstacle.  In general position these are the
 *                triangles at the origin of the planar Delaunay triangulation of {0} u {(X_a, Y_a)}.  partner [n,k] int32: partner[i,a]
 *                is the slot b of the triangle {a, b} with cr(a, b) > 0 (each triangle once, on its clockwise slot), or -1.  Co-circular
 *                points (in-circle exactly 0) are not inside: of two tied partners the lower slot is kept.
 *                status: one device int32, set to the number of rows that held an index outside [0,n); such a row reads nothing through
 *                it and has no triangle (all -1).  The caller reads the word at its next synchronisation point.
 *        emit    For every filled slot the lifted 3-D triangle (v0, v1, v2) = (i, nbr[i,a], nbr[i,b]): with cot_c = dot / |cross| at corner c
 *                and w_c = cot_c / 2 / 3, the edge opposite corner c gets -w_c on its two off-diagonals and +w_c on its two diagonals;
 *                every vertex gets area / 3 / 3 of mass (the second third: in the interior a triangle shows up in the stars of all three
 *                of its corners).  Written to the workspace (dn_cloud_laplacian_workspace_bytes(n, k) = 192 n k bytes), S = n k slots:
 *                  int64 key_l [9 S] at byte 0, fp64 val_l [9 S] at 72 S, int64 key_m [3 S] at 144 S, fp64 val_m [3 S] at 168 S;
 *                slot s = i k + a owns entries 9 s .. 9 s + 8 of L -- keys (row << 32 | col): the diagonals of v0, v1, v2 (each the sum of
 *                its two edge weights), then (v0,v1) (v1,v0) (v0,v2) (v2,v0) (v1,v2) (v2,v1) -- and 3 s .. 3 s + 2 of the mass (keys v0,
 *                v1, v2).  An empty slot (partner -1 or out of range, an index out of range, a lifted triangle without area) writes the
 *                key INT64_MAX, which sorts last, and the value 0.
 *        sum     dn_segment_sum_f64_f32 on keys [m] sorted ascending by a STABLE sort, perm [m] int64 (position of each sorted key
 *                in the unsorted arrays), vals [m] fp64 (unsorted): every run of equal keys other than INT64_MAX is added in sorted order
 *                in fp64 and rounded to fp32 once.  rowptr != NULL: keys are (row << 32 | col) with row, col in [0, n_rows); rank [m] int64
 *                is the inclusive count of run heads (keys[p] != keys[p-1]) up to p; the r-th run goes to col[r], out[r] (both [m]),
 *                rowptr [n_rows + 1] is filled and *count (device int32) set to the number of runs: CSR with ascending columns.
 *                rowptr == NULL (col, rank, count unused): keys index out [n_rows], which is zeroed first.
 *      L = sum over all stars is symmetric with zero row sums and positive semi-definite for ANY input (a sum of per-triangle Dirichlet
 *      forms); without the intrinsic re-triangulation single weights can be negative on bad samplings.  Everything from the coordinate
 *      differences on is fp64.  No floating-point atomics: the result is bit-identical from run to run, and entries (i,j) and (j,i)
 *      are sums of the same terms in the same order -- the same bits.
 *      Each returns 0 on success (n == 0, or m == 0 and n_rows == 0: nothing is launched) and non-zero WITHOUT launching for k < 1,
 *      k > DN_KNN_MAX_K, n < 0, 9 n k > INT32_MAX (the query returns 0 bytes for these), m < 0, n_rows < 0, a workspace smaller than
 *      the query says, or a NULL pointer that the call would use. */
size_t dn_cloud_laplacian_workspace_bytes(int n, int k);
int dn_cloud_star_f32(const float* pts, int n, const int64_t* nbr, int k, const float* frames, int32_t* partner, int32_t* status, void* stream);
int dn_cloud_laplacian_emit_f32(const float* pts, int n, const int64_t* nbr, int k, const int32_t* partner, void* ws, size_t ws_bytes,
                                void* stream);
int dn_segment_sum_f64_f32(const int64_t* keys, const int64_t* perm, const double* vals, int m, const int64_t* rank, int n_rows,
                           int32_t* rowptr, int32_t* col, float* out, int32_t* count, void* stream);

/* ---- triangle-mesh operators (geometry.py:114-148, 151-177, 209-273, 306-335 for a mesh; dn_mesh.hip): cotan Laplacian, lumped mass,
 *      vertex normal sums, tangent frames and the least-squares gradient operator.  verts [n_verts,3] fp32; faces [n_faces,3] int64.
 *        emit    dn_mesh_emit_f32, one lane per face (v0, v1, v2).  Per corner o with opposite edge (i, j): a = x_i - x_o, b = x_j - x_o,
 *                w_o = 0.5 (a.b) / (|a x b| + 1e-10); the edge gets -w_o on its two off-diagonals and +w_o on its two diagonals.  Every
 *                vertex of the face gets a record (area / 3, n / (|n| + 1e-6)) with n = (x_1 - x_0) x (x_2 - x_0), area = |n| / 2 (the
 *                reference's normalize(): deliberately not quite unit).  Written to the workspace, dn_mesh_workspace_bytes(n_verts,
 *                n_faces) = 264 Fe bytes with Fe = n_faces rounded up to even (every array starts on a 16-byte boundary):
 *                  int64 key_l [9 F] at byte 0, fp64 val_l [9 F] at 72 Fe, int64 key_v [3 F] at 144 Fe, fp64 val_v [3 F, 4] at 168 Fe;
 *                face f owns entries 9 f .. 9 f + 8 of L -- keys (row << 32 | col): the diagonals of v0, v1, v2 (each the sum of its two
 *                edge weights: w_1 + w_2, w_2 + w_0, w_0 + w_1), then (v1,v2) (v2,v1) with -w_0, (v2,v0) (v0,v2) with -w_1, (v0,v1)
 *                (v1,v0) with -w_2 -- and records 3 f .. 3 f + 2 (keys v0, v1, v2, four values each: area / 3 and the unit normal).
 *                A face that repeats an index emits its terms as the formulas give them (a = 0, so w = 0): explicit zeros stay entries.
 *                status: one device int32, set to the number of faces that hold an index outside [0, n_verts); such a face reads nothing
 *                through it and writes the key INT64_MAX, which sorts last, and zeros.  The caller reads the word at its next
 *                synchronisation point.
 *        sum     dn_segment_sum_f64_f64: dn_segment_sum_f64_f32 with an fp64 `out` -- every run of equal keys (sorted ascending by a
 *                STABLE sort) other than INT64_MAX is added in sorted order in fp64 and stored as it is; rowptr != NULL: CSR with ascending
 *                columns (rank, col, count as there), rowptr == NULL: keys index out [n_rows], zeroed first.  dn_segment_sum4_f64_f64:
 *                the dense form for FOUR values per key, vals [m, 4] (unsorted) -> out [n_rows, 4]: the records of the vertices.
 *        vertex  dn_mesh_frames_gradients_f64, one lane per row of a CSR pattern (rowptr [n_verts + 1], col [nnz], int32; L's own) with
 *                normals [n_verts,3] fp64.  frames [n_verts,3,3] fp64, rows basisX, basisY, normal: basisX = c - n (n.c) with c = e_x where
 *                |n_x| < 0.9, else e_y, divided by (|basisX| + 1e-6); basisY = n x basisX.  Over the off-diagonal entries j of row i in
 *                column order: t_j = ((x_j - x_i).basisX, (x_j - x_i).basisY), G = sum_j t_j t_j^T + 1e-5 I; gx [nnz], gy [nnz] fp64 on
 *                the same pattern get G^-1 t_j at entry j and -sum_j G^-1 t_j at the diagonal entry.  An empty row writes its frame only.
 *                status: one device int32, set to the number of rows with a row pointer outside [0, nnz] or decreasing (nothing is walked),
 *                a column outside [0, n_verts) (its entry gets 0 and takes no part) or, if not empty, no diagonal entry.
 *      Everything from the coordinate differences on is fp64.  No floating-point atomics: every sum runs in the sorted order -- face
 *      after face, a face's terms in the order above -- so the result is bit-identical from run to run, and L[i,j] and L[j,i] are sums
 *      of the same terms in the same order: the same bits.
 *      Each returns 0 on success (n_faces == 0, n_verts == 0 with nnz == 0, or m == 0 and n_rows == 0: nothing is launched and nothing
 *      is written, the status word included) and non-zero WITHOUT launching for n_verts < 0, n_faces < 0, 9 n_faces > INT32_MAX (the query
 *      returns 0 bytes for these), nnz < 0, nnz > 0 with n_verts == 0, m < 0, n_rows < 0, a workspace smaller than the query says, or a
 *      NULL pointer that the call would use. */
size_t dn_mesh_workspace_bytes(int n_verts, int n_faces);
int dn_mesh_emit_f32(const float* verts, int n_verts, const int64_t* faces, int n_faces, void* ws, size_t ws_bytes, int32_t* status, void* stream);
int dn_segment_sum_f64_f64(const int64_t* keys, const int64_t* perm, const double* vals, int m, const int64_t* rank, int n_rows,
                           int32_t* rowptr, int32_t* col, double* out, int32_t* count, void* stream);
int dn_segment_sum4_f64_f64(const int64_t* keys, const int64_t* perm, const double* vals, int m, int n_rows, double* out, void* stream);
int dn_mesh_frames_gradients_f64(const float* verts, int n_verts, const int32_t* rowptr, const int32_t* col, int nnz, const double* normals,
                                 double* frames, double* gx, double* gy, int32_t* status, void* stream);

/* ---- functional maps (experiments/functional_correspondence/fmaps_model.py:11-40): the regularised spectral solve and its backward
 *      (dn_fmap.hip).  A, B [P, K, F] fp32 row-major: the spectral coefficients of the features of shapes x and y of P pairs;
 *      evals_x, evals_y [P, K] fp32; lam: the regularisation weight.  With G = A A^T, H = B A^T and
 *      D_i = diag_j (evals_x[j] - evals_y[i])^2, row i of C [P, K, K] is
 *          c_i = (G + lam D_i)^-1 H[i, :]^T
 *      -- K symmetric positive (semi-)definite K x K systems that share G, each factored once by Cholesky without pivoting.
 *      bwd: with dC [P, K, K] = dL/dC, u_i = (G + lam D_i)^-1 dC[i, :]^T, U the matrix of rows u_i^T and dG = -U^T C:
 *          dA = (dG + dG^T) A + U^T B,   dB = U A      ([P, K, F] fp32; no gradient for the eigenvalues or lam).
 *      bwd recomputes G, the factorisations and c_i from A, B and the eigenvalues: it takes no stored C, whose fp32 rounding would
 *      enter the gradient.
 *      Operands and results are fp32; everything from the loads on is fp64 (lam is widened as it is), rounded once at the store.  No
 *      float atomics: the result is bit-identical from run to run.  Two launches forward, three backward, no host synchronisation.
 *      A pivot that is not a positive finite number (a singular system, a non-finite operand) faults nothing and reads nothing outside the
 *      matrix: fwd stores that row of C as NaN, bwd stores NaN in all of that pair's dA and dB.  status (may be NULL): one device int32
 *      that the call first sets to 0 and then raises by one for every such row; the caller reads it at its next synchronisation point.
 *      Workspace: dn_fmap_workspace_bytes(P, K, F) bytes serve either direction (G, H, and for bwd C and U, in fp64).
 *      Returns 0 on success (P == 0: nothing is launched) and non-zero WITHOUT launching for K < 1, K > DN_FMAP_MAX_K, F < 1 (or
 *      F > 65535 * 32), P < 0, a NULL operand, result or workspace while P > 0, or a workspace smaller than the query says. */
#define DN_FMAP_MAX_K 64
int dn_fmap_max_k(void);
size_t dn_fmap_workspace_bytes(int P, int K, int F);
int dn_fmap_solve_fwd_f32(const float* A, const float* B, const float* evals_x, const float* evals_y, int P, int K, int F, float lam, float* C,
                          void* ws, size_t ws_bytes, int32_t* status, void* stream);
int dn_fmap_solve_bwd_f32(const float* A, const float* B, const float* evals_x, const float* evals_y, const float* dC, int P, int K, int F, float lam,
                          float* dA, float* dB, void* ws, size_t ws_bytes, int32_t* status, void* stream);

/* ---- all-pairs mesh distances (geometry.geodesic_label_errors, geometry.py:754-896): (min, +) relaxation sweeps of a block of distance
 *      columns over a graph (dn_geodesic.hip).  rowptr [n_nodes + 1], col [nnz] int32: the CSR arcs of every node, columns in [0, n_nodes)
 *      (NOT checked here: the caller validates them); w [nnz] fp64 arc lengths, non-negative and not NaN.  dist [n_nodes, n_src] fp64,
 *      NODE-major: column s holds the distances from source s, which the caller initialises (inf, 0 at the source).  One sweep is
 *          dist[v][s] = min(dist[v][s], dist[u][s] + w)   over every arc (u, w) of row v, every v and every s,
 *      one fp64 add per arc and nothing reassociated.  The call runs n_sweeps sweeps IN PLACE, one launch each: values only decrease and
 *      each is the length of a path, so the fixed point -- the minimum over paths of the left-to-right fp64 sum, what Dijkstra returns --
 *      does not depend on the order in which lanes see each other's stores; how many sweeps reach it may.  Any n_src (lanes are masked,
 *      nothing is padded), any n_nodes, empty rows and rows of any length are handled.
 *      changed: one device int32 that the call first sets to 0 and then sets to 1 if its LAST sweep lowered any value; 0 after a call with
 *      n_sweeps >= 1 therefore certifies the fixed point.  The caller reads it at its next synchronisation point.
 *      No workspace, no allocation, no synchronisation.  dn_minplus_node_tile(): the nodes a workgroup owns (for tests of ragged sizes).
 *      Returns 0 on success (n_nodes, n_src or n_sweeps == 0: only the word is cleared) and non-zero WITHOUT launching for a negative
 *      count, a NULL changed, a NULL rowptr or dist otherwise, or n_src > 65535 * 64. */
int dn_minplus_node_tile(void);
int dn_minplus_sweeps_f64(const int32_t* rowptr, const int32_t* col, const double* w, int n_nodes, double* dist, int n_src, int n_sweeps,
                          int32_t* changed, void* stream);

/* ---- Laplacian eigenbasis (geometry.laplacian_eigenbasis): one step of the Chebyshev recurrence on a block of vectors (dn_eigen.hip),
 *      every product with S of the filtered subspace iteration.  rowptr [n_rows + 1], col [nnz] int32, val [nnz] fp64: S in CSR, columns in
 *      [0, n_rows) (NOT checked here: the caller validates them).  Y, Z, out: fp64 row-major blocks [n_rows, ld] of which columns [0, nb)
 *      are used, ld >= nb.
 *          out[i][c] = alpha * sum_p val[p] * Y[col[p]][c]  +  beta * Y[i][c]  +  gamma * Z[i][c]     p in [rowptr[i], rowptr[i + 1])
 *      (1, 0, 0) is S Y; (2 / e, -2 c / e, -1) with Z the block before last is one step of T_(j+1) = 2 ((S - c) / e) T_j - T_(j-1).
 *      One fma per entry in CSR order, then alpha * sum, fma(beta, Y, .), fma(gamma, Z, .); no atomics: repeatable bit for bit.  A term
 *      whose scalar is 0 is not formed and its operand not read: Z may be NULL when gamma == 0.  out may be Z (each element is read by the
 *      lane that writes it); out must not be Y.  Columns [nb, ld) are never read from Y or Z and never written in out.  Any nb (64-column
 *      tiles, lanes masked), any n_rows, empty rows and rows of any length.  No workspace, no allocation, no synchronisation.
 *      dn_cheb_rows_per_workgroup(): the rows a workgroup owns (for tests of ragged sizes).
 *      Returns 0 on success (n_rows == 0 or nb == 0: nothing is launched) and non-zero WITHOUT launching for a negative size, ld < nb, a
 *      NULL rowptr, col, val, Y or out, a NULL Z with gamma != 0, out == Y, or nb > 65535 * 64. */
int dn_cheb_rows_per_workgroup(void);
int dn_cheb_step_f64(const int32_t* rowptr, const int32_t* col, const double* val, int n_rows, const double* Y, const double* Z, double* out,
                     int nb, int ld, double alpha, double beta, double gamma, void* stream);

/* ---- implicit diffusion (LearnedTimeDiffusion, method 'implicit_sparse'; reference layers.py:69-84 without the dense matrix): for every
 *      mesh b and channel c the system (diag(m_b) + t_c L_b) x_bc = b_bc by Jacobi-preconditioned conjugate gradients (dn_implicit.hip).
 *      rowptr [v_total + 1], col [nnz] int32, val [nnz] fp32: L in CSR over the concatenated vertex axis, block diagonal over the meshes,
 *      columns in [0, v_total) (NOT checked here: the caller validates them); mass [v_total], time [C] (already clamped) fp32.
 *      tiles [n_tiles][4] int32 (row0, nrows, mesh, 0) and mesh_tile_off [n_mesh + 1] int32, on the device: runs of at most
 *      dn_implicit_rows_per_tile() rows of ONE mesh that cover [0, v_total) in order, and the first tile of every mesh (every mesh has at
 *      least one row).  A tile is cut to the rows that exist: a wrong table gives wrong numbers, never an access outside the operands.
 *      The blocks rhs, x0, out, x are fp32 row-major [v_total][C], contiguous.  All solver state (x, r, p, q, dot products, scalars) is
 *      fp64 in the workspace, which the four calls of one solve share: dn_implicit_workspace_bytes(v_total, C, n_tiles, n_mesh) bytes.
 *        init     b = m (.) rhs (rhs_mass != 0) or rhs; x = x0, or with x0 NULL b / m; r = b - A x, p = r / d, d = m + t diag(L) (the
 *                 diagonal found by scanning each row; an empty row gives d = m); a system with ||r|| <= rtol ||b|| is done at once.
 *        iterate  n_iter iterations, four launches each: q = A p and p.q | alpha, x += alpha p, r -= alpha q, r.z and r.r | beta, the
 *                 iteration count, done | p = r / d + beta p.  Norms and dot products are per (mesh, channel), over that mesh's rows, summed
 *                 in one fixed order without atomics: results repeat bit for bit.  A done system is frozen: further iterations change no
 *                 bit of it.  A NaN or inf stays in its (mesh, channel).  unfinished: one device int32 that receives the number of systems
 *                 not done after the call (n_iter == 0: only this); the caller reads it at its next synchronisation point.
 *        finish   out = fp32(x), or fp32(m (.) x) with out_mass != 0; iterations [n_mesh][C] int32 and residual [n_mesh][C] fp64, the
 *                 final ||r|| / ||b|| of the recurrence (either may be NULL).
 *        lx_dot   d_time[c] = - sum over meshes, in mesh order, of g_bc . (L_b x_bc) with g the fp64 solution the workspace holds (the
 *                 backward's solve) and x an fp32 block: the gradient of the diffusion times.
 *      No allocation, no synchronisation, no memset nodes, no environment.  Every call returns 0 on success (v_total == 0 or C == 0:
 *      nothing is launched, except that lx_dot with v_total == 0 stores zeros) and non-zero WITHOUT launching for a negative size, a NULL
 *      required pointer, a workspace smaller than the query says, C > 65535 * 64, a tile table that cannot cover v_total (n_tiles *
 *      dn_implicit_rows_per_tile() < v_total, n_tiles > v_total, or n_mesh > n_tiles), a negative or NaN rtol. */
int dn_implicit_rows_per_tile(void);
size_t dn_implicit_workspace_bytes(int v_total, int C, int n_tiles, int n_mesh);
int dn_implicit_init_f32(const int32_t* rowptr, const int32_t* col, const float* val, const float* mass, const float* time, const int32_t* tiles,
                         int n_tiles, const int32_t* mesh_tile_off, int n_mesh, int v_total, int C, const float* rhs, int rhs_mass, const float* x0,
                         double rtol, void* ws, size_t ws_bytes, void* stream);
int dn_implicit_iterate_f32(const int32_t* rowptr, const int32_t* col, const float* val, const float* mass, const float* time, const int32_t* tiles,
                            int n_tiles, const int32_t* mesh_tile_off, int n_mesh, int v_total, int C, int n_iter, int32_t* unfinished, void* ws,
                            size_t ws_bytes, void* stream);
int dn_implicit_finish_f32(const float* mass, const int32_t* tiles, int n_tiles, const int32_t* mesh_tile_off, int n_mesh, int v_total, int C,
                           int out_mass, float* out, int32_t* iterations, double* residual, void* ws, size_t ws_bytes, void* stream);
int dn_implicit_lx_dot_f32(const int32_t* rowptr, const int32_t* col, const float* val, const int32_t* tiles, int n_tiles,
                           const int32_t* mesh_tile_off, int n_mesh, int v_total, int C, const float* x, float* d_time, void* ws, size_t ws_bytes,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFNET_HIP_H */
