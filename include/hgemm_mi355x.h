/*
 * hgemm_mi355x.h -- C ABI of libhgemm_mi355x.so, the MI355X (gfx950/CDNA4) HGEMM library that
 * replaces the hot path of deepreinforce-ai/CUDA-L2:
 *
 *     C[M,N] (fp16) = A[M,K] (fp16) x B[K,N] (fp16),  fp32 accumulate, alpha = 1, beta = 0
 *
 * Two calls add an existing bf16 matrix to the product (beta = 1, in place if wished): bgemm_mi355x_tn_bias_add and bgemm_mi355x_nn_add,
 * the two ends of a residual block; the fp32 C of the _ta_c32 calls accumulates.  Every other entry point computes beta = 0.
 *
 * Everything here is `extern "C"`, plain pointers and ints; no torch types.  The torch
 * extension `hgemm_lib` (cuda-l2_amd/pybind/hgemm_mi355x_{fp16,fp32}.cc) is a thin shim over
 * these entry points and exports the 15 Python names the reference harness binds
 * (reference pybind/hgemm_a100_fp32.cc:29-52).  INTEGRATION.md shows the binding.
 *
 * Conventions shared by every GEMM entry point
 *   a            device pointer, fp16 [M][K] row-major contiguous
 *   b            device pointer, fp16 [K][N] row-major contiguous
 *   b_col_major  device pointer, fp16 [N][K] row-major contiguous (= B transposed; the
 *                reference harness builds it with tools/utils.py:110-115 as_col_major)
 *   c            device pointer, fp16 [M][N] row-major contiguous, overwritten
 *   stream       hipStream_t (NULL = the legacy default stream, which is what the reference's
 *                <<<grid,block,smem>>> launches use, kernels/a100_F32F16F16F32/64_4096_64.cu:263)
 *   return       0 on success, a negative hgemm_status_t otherwise; launches are asynchronous,
 *                device faults surface at the caller's next synchronisation (same as the
 *                reference, zero_one_correctness_check.py:161-165).
 * Ownership: the caller owns all buffers; the library keeps no pointer past the call.
 */
#ifndef HGEMM_MI355X_H_
#define HGEMM_MI355X_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  HGEMM_OK = 0,
  HGEMM_ERR_BAD_ARG = -1,     /* null pointer, non-positive dimension, bad id */
  HGEMM_ERR_TOO_LARGE = -2,   /* a dimension exceeds the 32-bit addressing of one operand */
  HGEMM_ERR_HIP = -3,         /* a HIP runtime call failed (see hgemm_mi355x_last_hip_error) */
  HGEMM_ERR_BACKEND = -4,     /* rocBLAS / hipBLASLt returned an error */
  HGEMM_ERR_NOT_READY = -5,   /* baseline used before its init / find_best call */
  HGEMM_ERR_NO_ALGO = -6,     /* hipBLASLt returned no usable algorithm */
  HGEMM_ERR_NO_WORKSPACE = -7 /* hgemm_mi355x_reserve_workspace only: lent buffer too small, out of memory, or the
                                 stream is capturing (a GEMM call never returns it: it runs without split-K instead) */
} hgemm_status_t;

/* Accumulate mode names the reference's two kernel trees (F32F16F16F32 / F16F16F16F16).
 * CDNA4 has no fp16-accumulating MFMA (all f16 MFMA opcodes are v_mfma_f32_*), so both modes
 * run the same fp32-accumulate kernels here; for the rocBLAS / hipBLASLt baselines the mode
 * selects the compute type exactly as the reference's cublas/fp16 vs cublas/fp32 trees do. */
typedef enum { HGEMM_ACC_FP32 = 0, HGEMM_ACC_FP16 = 1 } hgemm_acc_t;

/* Special config ids of hgemm_mi355x_launch / hgemm_mi355x_plan (ids >= 0 index the geometry table of THIS library build:
 * resolve a geometry by name with hgemm_mi355x_config_by_name, ids shift when a build adds members). */
#define HGEMM_CONFIG_GENERIC (-1) /* one-output-per-thread reference kernel; reads b (row-major)        */
#define HGEMM_CONFIG_RAGGED  (-2) /* register-staged MFMA kernel for any M,N,K / alignment; reads b_col_major */

/* Split-K forms.  `splits` > 1 selects the two-launch form: fp32 slabs [splits][M][N] + a combine kernel that
 * adds them in split order.  OR-ing HGEMM_SPLITK_FUSED into `splits` selects the single-launch form instead
 * (fp32 partials + a per-tile arrival counter; the last workgroup to arrive adds the partials in split order
 * and writes the tile -- the deterministic counterpart of the reference's atomicAdd split-K,
 * kernels/a100_F32F16F16F32/64_256_16384.cu:149-152).  Measured on MI355X the single-launch form only wins
 * for the very smallest outputs (the last arriver reads the slabs alone, at 60-110 GB/s), so the tuner picks
 * it per shape.  Both forms are deterministic (fixed summation order). */
#define HGEMM_SPLITK_FUSED 0x10000
#define HGEMM_SPLITK_MASK  0x0ffff
/* Plan flag, OR-ed into `splits` like HGEMM_SPLITK_FUSED: the fp16 C stores of the launch are non-temporal (streaming).
 * C is written once and never re-read; streaming stores leave the device during the epilogue instead of sitting dirty in
 * the XCDs' write-back L2s until the end-of-kernel release.  Measured back to back on MI355X (round 3): the gap between
 * two launches shrinks from 3.7 to 2.0 us; 4096^3 -4 %, 8192 x 16384 x 256 -8 %, 16384^2 x 256 +1.5 %: the tuner decides
 * per shape.  Results are bit-identical either way.
 * Honoured by the direct fp16 epilogues of every family (whole tiles of a stream-K run and the last arriver of a single-launch
 * split-K included); ignored by the two-pass combine kernel, the hybrid tail's reduce and the any-shape kernels; the off-grid
 * planner does not propagate it from a corner plan. */
#define HGEMM_PLAN_NT_STORE 0x20000
/* Plan flag: STREAM-K (the reference's H100 tree: cutlass::gemm::StreamKScheduler, kernels/h100_F32F16F16F32/
 * 128_4096_16384.cu:79, 16384_512_2048.cu:71-73).  One persistent launch: the tiles x K-stages of the GEMM form one
 * tile-major sequence and each of G workgroups walks a contiguous run of it, so the chip is filled whatever the tile count
 * (12288 x 128 x 8192: 96 tiles of 128 x 128 on 256 CUs) and the workgroups of a cut tile start their K walks at different
 * offsets.  With the flag the low 16 bits of `splits` are G (0 or 1: one resident wave of workgroups, 256 x the geometry's
 * workgroups per CU).  At most the first and the last segment of a run are partial tiles; they go through compact fp32
 * slabs and per-tile arrival counters, the workgroup that completes a tile adds its parts in K order (deterministic, nobody
 * waits).  Geometries of the classic ("t") and register-staged ("r") families have the kernel
 * (hgemm_mi355x_config_streamk); elsewhere, or without workspace, the plan runs as the geometry's plain launch. */
#define HGEMM_PLAN_STREAMK 0x40000
/* LOCAL split (family "u", names u<BM>x<BN>_w<WM>x<WN>_k4): the one way of putting several wave sets on the K walk of ONE output
 * tile that does not go through HBM.  The workgroup is WM x WN x 4 waves; a pipeline stage (128 or 256 of K:
 * hgemm_mi355x_config_k_granularity) is staged into LDS by all sixteen waves, K-group g runs the MFMAs of its quarter of the stage,
 * and after the walk the four groups' fp32 accumulators are added through LDS in group order 0, 1, 2, 3 (fixed: deterministic per
 * plan), rounded once to fp16 and stored by all waves.  One launch, no slabs, no counters, no workspace -- so a `splits` = 1 plan of
 * the family can be captured into a hipGraph without a reserved workspace.  An external `splits` > 1 composes with it (two-pass form:
 * the slab is written after the LDS reduce); HGEMM_SPLITK_FUSED on such a geometry runs as the two-pass form and HGEMM_PLAN_STREAMK
 * as its plain launch (it has neither kernel); HGEMM_PLAN_NT_STORE is honoured.  K must be a whole number of stages, any other K is
 * served by the any-shape kernel (HGEMM_OK, exact).  Explicit plans only: hgemm_mi355x_plan, the off-grid rules and the first-use
 * candidates never return a family-u geometry.  hgemm_mi355x_config_local_splits tells the factor. */

/* Plan flags of the register-staged streaming family ("r" geometries; ignored elsewhere).  Results are exact either way (0/1
 * inputs) / differ only in the summation order of a tile's K walk (N(0,1) inputs), deterministically per plan.
 * HGEMM_PLAN_RS_XCD_STAGGER: the K stagger of the family (workgroups start their K walk at different stages so that the chip does
 *   not read one K offset of rows 16-32 KiB apart at the same time) is taken per XCD instead of per tile: the workgroups of an
 *   XCD walk K in lock-step and share the slices of the small operand in that XCD's L2; the eight XCDs are nk / 8 stages apart.
 *   (The summation order of a tile then depends on which workgroup computes it: "per plan" includes the raster group, as it does
 *   for a stream-K plan.)
 * HGEMM_PLAN_RS_NT_LOADS: the STREAMED operand (the one with more rows, read exactly once) is loaded non-temporally, so it does
 *   not push the shared operand's slices out of the L2 (what hipBLASLt's kernels do on the skinny shapes: NTA / NTB). */
#define HGEMM_PLAN_RS_XCD_STAGGER 0x80000
#define HGEMM_PLAN_RS_NT_LOADS    0x100000
/* The same bit for the "q" geometries (round 5; 16x16x32 members, K a whole number of pipeline stages -- ignored otherwise):
 * HGEMM_PLAN_XCD_STAGGER selects the "kstagger" kernel variant -- the workgroups of XCD x walk every work item's K stages in the
 * rotated order x nk / 8, ..., nk - 1, 0, ..., x nk / 8 - 1 (family q has no stagger without the flag).  For the one-round plans
 * whose 256 workgroups otherwise read the same K offset of rows 16-32 KiB apart at the same time: the reference's H100 tree
 * gets the same effect from stream-K start offsets (kernels/h100_F32F16F16F32/16384_512_2048.cu:71-73).  Exactness / determinism
 * as above. */
#define HGEMM_PLAN_XCD_STAGGER HGEMM_PLAN_RS_XCD_STAGGER
/* Plan flags of the persistent "q" geometries (round 5; ignored elsewhere).  Results are bit-identical with and without them.
 * HGEMM_PLAN_PHASE_OFFSET: every second workgroup of an XCD starts its walk over the work items half an item period late, so
 *   that the epilogues of an XCD's CUs (their C stores share the XCD's path into the fabric) no longer coincide.  For walks of
 *   several items per workgroup.
 * HGEMM_PLAN_WAVE_PRIORITY: two-resident members (two workgroups per CU: q128x128_w2x2, q192x128_w2x2, q128x192_w2x2): the two
 *   waves of a SIMD get different static priorities, so one workgroup's epilogue runs under the other's K loop. */
#define HGEMM_PLAN_PHASE_OFFSET  0x200000
#define HGEMM_PLAN_WAVE_PRIORITY 0x400000
#define HGEMM_PLAN_PHASE_OFFSET4 0x800000   /* four phase groups a quarter period apart instead of two half a period apart */
#define HGEMM_PLAN_PHASE_OFFSET8 (HGEMM_PLAN_PHASE_OFFSET | HGEMM_PLAN_PHASE_OFFSET4)   /* both bits: eight groups an eighth of a period apart */

/* ------------------------------------------------------------------------------------------
 * The hot path.  Replaces cuda_l2_<dev>_fp32(a, b, b_col_major, c)
 * (reference kernels/a100_F32F16F16F32/64_4096_64.cu:275-287) and cuda_l2_<dev>_fp16
 * (kernels/a100_F16F16F16F16/4096_4096_4096.cu:280-295).  Picks the tuned kernel geometry /
 * split-K plan for (M,N,K) and launches it: the tuned table for the 1000 grid shapes; for any other shape the
 * tuned plans of the grid shapes around it, ranked by the analytic model (the model alone when none of them fits);
 * off-grid plans are remembered per thread, so a repeated shape costs one table probe.
 * Any M,N,K >= 1 is accepted; shapes the LDS-DMA kernels cannot take (K % 8 != 0, N % 4 != 0,
 * pointers or strides not 16-byte aligned, operands beyond 32-bit tile offsets) run on a register-staged
 * MFMA kernel that pads on the way into LDS (the reference pads in the harness, tools/utils.py:8-36).
 * Thread / stream safety: calls may be issued from any thread on any stream and device; split-K plans use
 * a library-owned workspace that is private to the (device, stream) pair of the call. */
int hgemm_mi355x_fp32(const void* a, const void* b, const void* b_col_major, void* c,
                      int M, int N, int K, void* stream);
int hgemm_mi355x_fp16(const void* a, const void* b, const void* b_col_major, void* c,
                      int M, int N, int K, void* stream);

/* Explicit-plan launch: what a per-shape kernel file
 * (cuda-l2_amd/kernels/mi355x_<acc>/<M>_<N>_<K>.hip, the analogue of the reference's
 * kernels/<dev>_<acc>/<M>_<N>_<K>.cu) and the autotuner call.
 *   config_id  index into the geometry table (hgemm_mi355x_config_*), HGEMM_CONFIG_GENERIC or
 *              HGEMM_CONFIG_RAGGED; a table geometry whose alignment rules the operands do not meet is
 *              served by the ragged kernel
 *   splits     split-K factor >= 1, optionally | HGEMM_SPLITK_FUSED (see above); clamped to K / 64;
 *              degrades to 1 when no workspace is available (lent buffer too small, out of memory)
 *   group_m    rasterisation group height in tiles (>= 1)
 * lda/ldb/ldc are row strides in elements: lda of a (>= K), ldb of b_col_major (>= K; unused without b_col_major), ldc of c
 * (>= N); a smaller stride (zero and negative ones included) returns HGEMM_ERR_BAD_ARG.  The row-major b is always read at
 * stride N. */
int hgemm_mi355x_launch(int config_id, int splits, int group_m,
                        const void* a, const void* b, const void* b_col_major, void* c,
                        int M, int N, int K, int lda, int ldb, int ldc, void* stream);

/* First-use plan selection on the box the library runs on (opt-in; the reference's H100 kernels time their variants on first
 * invocation, kernels/h100_F32F16F16F32/64_4096_64.cu:623-690).  Off by default: the entry points take the tuned table's plan.
 * With HGEMM_MI355X_INSITU=1 in the environment, or after hgemm_mi355x_set_insitu(1) (returns the previous setting; 0 also
 * forgets every recorded choice), the FIRST call of hgemm_mi355x_fp32 / _fp16 for a shape times up to three oracle-verified
 * plans -- the table's and its alternates (hgemm_mi355x_insitu_candidates lists them, the table's plan first; off the grid, round 6:
 * the planner's plan, then the runners-up among the tuned plans of the surrounding grid shapes in the model's order) -- on the call's
 * own operands and stream (interleaved rounds), keeps the fastest for the (process, device) (an alternate must win by 3 %) and runs it; that call
 * synchronises the stream, so it belongs in a warm-up phase.  Later calls, and calls on a capturing stream, time nothing.
 * hgemm_mi355x_insitu_choice returns 1 and the recorded plan once a shape has been measured. */
int hgemm_mi355x_set_insitu(int enable);
/* 1 when first-use selection is on (environment or hgemm_mi355x_set_insitu).  The per-shape kernel files
 * (csrc/hgemm_shape_entry.hpp) ask this before they launch their pinned plan: with the selection on they hand the call to
 * hgemm_mi355x_fp32 / _fp16 instead, so that `HGEMM_MI355X_INSITU=1 ./eval_one_file.sh ...` (or `--insitu`) measures on the
 * harness path -- where the reference's first-call autotune runs (kernels/h100_F32F16F16F32/64_4096_64.cu:702-721).
 * Choices are kept per (device, shape).  With the selection on, N(0,1) results may differ in their last bits from run to run and box
 * to box: a split-K / K-stagger alternate adds a tile's K stages up in another (fixed, deterministic per plan) order; 0/1 inputs
 * stay exact whatever is chosen. */
int hgemm_mi355x_insitu_enabled(void);
int hgemm_mi355x_insitu_candidates(int M, int N, int K, int config_id[3], int splits[3], int group_m[3]);
int hgemm_mi355x_insitu_choice(int M, int N, int K, int* config_id, int* splits, int* group_m);

/* Plan the library would use for (M,N,K): outputs config id, split-K factor, raster group. */
int hgemm_mi355x_plan(int M, int N, int K, int* config_id, int* splits, int* group_m);

/* The analytic cost model behind hgemm_mi355x_plan, exposed for the autotuner's candidate
 * pruning and for reports: estimated microseconds of (config_id, splits) on (M,N,K). */
double hgemm_mi355x_model_us(int config_id, int splits, int M, int N, int K);

/* Raster group height the planner uses for (config, M, N) when no tuned value exists. */
int hgemm_mi355x_default_group(int config_id, int M, int N);

/* Geometry table introspection (ids are stable positions in csrc/hgemm_configs.def). */
int hgemm_mi355x_num_configs(void);
const char* hgemm_mi355x_config_name(int config_id);
/* out[0..7] = BM, BN, WM, WN, MI, NBUF, threads, lds_bytes */
int hgemm_mi355x_config_info(int config_id, int out[8]);
int hgemm_mi355x_config_by_name(const char* name);
/* The K multiple a geometry accepts: 8 for the families that take a K tail -- the classic "t" family zero-fills a partial
 * last K-step itself; families "q" (16x16x32 members) and "r" run the whole pipeline stages and accumulate the remainder
 * from fragments loaded straight from global memory (round 4; K must then hold at least one whole stage:
 * hgemm_mi355x_config_accepts_k) -- and the pipeline stage depth for the others (64; the reference pads K in the
 * harness instead, tools/utils.py:8-36).  hgemm_mi355x_launch returns HGEMM_ERR_BAD_ARG for a table geometry when K is a
 * multiple of 64 but not of its stage depth (family u excepted: every K it cannot take goes to the any-shape kernel), and serves
 * any other K it cannot take with the any-shape kernel (the planner never picks such a geometry); 1 for the special ids. */
int hgemm_mi355x_config_k_granularity(int config_id);
/* 1 when hgemm_mi355x_launch runs this geometry's own kernel for a problem with this K (operands aligned), 0 when it
 * would fall back or refuse: K a multiple of the stage depth, or K % 8 == 0 on a geometry with a K tail (families q and
 * r: K >= one stage). */
int hgemm_mi355x_config_accepts_k(int config_id, int K);
/* K-groups INSIDE the geometry's workgroup (the local split above): 4 for family u, 1 for every other table geometry, -1 for an
 * id outside the table. */
int hgemm_mi355x_config_local_splits(int config_id);
/* > 0 when the geometry has a stream-K kernel (HGEMM_PLAN_STREAMK): workgroups of it one CU holds. */
int hgemm_mi355x_config_streamk(int config_id);
/* 1 when a HGEMM_PLAN_STREAMK plan of this geometry really runs as stream-K on (M, N, K) -- the family has the kernel, K has no
 * direct tail, the tile count fits the arrival-counter block -- 0 when hgemm_mi355x_launch would run the geometry's plain
 * data-parallel launch instead (it still returns HGEMM_OK: a degraded plan is a slower plan, not an error).  Tuners and
 * candidate generators ask this before they record a "stream-K" timing. */
int hgemm_mi355x_streamk_runs(int config_id, int M, int N, int K);

/* Split-K workspace.  Default: the library keeps one private device buffer per (device, stream) pair that
 * issued a split-K plan and grows it on first use of a bigger plan only (never in steady state; growing
 * frees the old buffer with hipFree, which synchronises the device).  Concurrent GEMMs on different streams
 * or devices therefore never share partial sums.
 * hgemm_mi355x_set_workspace lends ONE caller-owned buffer instead (NULL returns to the default): it is
 * bound to the device that is current at the call, used for every stream of that device -- so the caller
 * must not run split-K GEMMs concurrently on several streams while it is lent -- and its first 256 KiB are
 * zeroed here (tile arrival counters).  A plan that does not fit the lent buffer runs with splits = 1.
 * hgemm_mi355x_workspace_bytes gives a sufficient size for (M, N, splits); hgemm_mi355x_release_workspaces
 * frees the library-owned buffers (call with no GEMM in flight and no hipGraph that holds one still alive).
 *
 * hipGraph capture (launch-bound shapes: a 64x4096x64 call is ~3 us of kernel behind ~7 us of launch): every
 * entry point may be called on a capturing stream -- the call records kernel nodes only, nothing is allocated,
 * synchronised or memset during capture.  A split-K (or hybrid-tail) plan needs its workspace to exist before
 * the capture starts: call hgemm_mi355x_reserve_workspace(M, N, K, stream) for the largest shape that will be
 * captured on that stream (or run the shape once on it); otherwise the captured call runs with splits = 1.
 * A buffer that a capture has used is never freed by later growth (it is retired until
 * hgemm_mi355x_release_workspaces), so instantiated graphs stay valid.  Replays of graphs captured on one
 * stream share that stream's workspace: do not replay them concurrently on several streams.
 *
 * Cost and lifetime: a (device, stream) pair that ever ran a split-K / hybrid plan keeps its buffer (>= 8 MiB, grown
 * geometrically) until hgemm_mi355x_release_workspaces; destroying the stream frees nothing, so an application with many
 * short-lived streams calls hgemm_mi355x_release_stream_workspace(stream) (current device, nothing of that stream in
 * flight) before hipStreamDestroy.  Allocation and growth switch the calling thread's stream-capture mode to relaxed
 * around hipMalloc / hipFree, so a capture that ANOTHER stream runs in global mode is not invalidated by them. */
int hgemm_mi355x_set_workspace(void* device_ptr, size_t bytes);
int hgemm_mi355x_release_stream_workspace(void* stream);
size_t hgemm_mi355x_workspace_bytes(int M, int N, int splits);
/* Exactly what hgemm_mi355x_launch asks for with this plan on (M, N, K) (0: none) -- the config-aware form: a stream-K plan needs
 * 2 x workgroups x BM x BN floats (a few MiB), where the geometry-blind bound above must assume 256 x 128 tiles and 1024 workgroups. */
size_t hgemm_mi355x_plan_workspace_bytes(int config_id, int splits, int M, int N, int K);
int hgemm_mi355x_reserve_workspace(int M, int N, int K, void* stream);
int hgemm_mi355x_release_workspaces(void);

/* ------------------------------------------------------------------------------------------
 * NN layout: C = A x B with B ROW-MAJOR ([K][N], as the conventions above call `b`), for the caller whose B is an activation and
 * has no pre-transposed copy to hand over.  Replaces what a b-only call of hgemm_mi355x_fp32 / _launch runs (the
 * one-output-per-thread reference kernel, HGEMM_CONFIG_GENERIC) and is the counterpart of the vendor baselines' _nn entry points
 * below (reference cublas/fp32/hgemm_cublas.cu:15-41, cublasGemmEx NN).  The kernels ("n" geometries, csrc/hgemm_kernel_nn.hpp) stage
 * B tiles row-major into LDS and read the MFMA operand through the hardware's transposed LDS read; they have a small table of their
 * own (ids 0 .. hgemm_mi355x_nn_num_configs() - 1, names n<BM>x<BN>_w<WM>x<WN>) that is separate from the geometry table above:
 * hgemm_mi355x_num_configs, the config ids and what the b_col_major entry points do are unchanged by it.
 * Scope of the kernels: K % 64 == 0, N % 8 == 0, lda / ldb / ldc multiples of 8, 16-byte aligned pointers, operands within 2 GiB of
 * 32-bit tile offsets.  Any other call is answered by the reference kernel: HGEMM_OK, exact, slow (hgemm_mi355x_nn_runs tells).
 *
 * hgemm_mi355x_nn_fp32 / _nn_fp16: the planned calls (both accumulate in fp32, as above); contiguous operands.
 * Replace cuda_l2_<dev>_fp32(a, b, b_col_major, c) (reference kernels/a100_F32F16F16F32/64_4096_64.cu:275-287) for a caller without
 * b_col_major. */
int hgemm_mi355x_nn_fp32(const void* a, const void* b, void* c, int M, int N, int K, void* stream);
int hgemm_mi355x_nn_fp16(const void* a, const void* b, void* c, int M, int N, int K, void* stream);
/* The explicit call (what hgemm_mi355x_launch is to the geometry table).
 *   nn_config  index into the NN table
 *   splits     split-K factor >= 1: the two-pass form (fp32 slabs [splits][M][N] + the combine kernel, added in split order:
 *              deterministic); clamped to K / 64; degrades to 1 when no workspace is available.  HGEMM_PLAN_NT_STORE is honoured;
 *              HGEMM_SPLITK_FUSED runs as the two-pass form and HGEMM_PLAN_STREAMK as the plain launch (the family has neither kernel)
 * lda (>= K), ldb (>= N: the row stride of the ROW-MAJOR b) and ldc (>= N) are in elements; a smaller stride returns
 * HGEMM_ERR_BAD_ARG, and so does an id outside the table.  Capturable on a stream like every entry point: a split plan needs its
 * workspace beforehand (hgemm_mi355x_nn_reserve_workspace, or hgemm_mi355x_reserve_workspace, whose floor of 64 MiB covers
 * splits x M x N x 4 bytes of most plans), otherwise the captured call runs unsplit. */
int hgemm_mi355x_launch_nn(int nn_config, int splits, const void* a, const void* b, void* c,
                           int M, int N, int K, int lda, int ldb, int ldc, void* stream);
/* The NN table (replaces nothing in the reference: it has one kernel file per shape). */
int hgemm_mi355x_nn_num_configs(void);
const char* hgemm_mi355x_nn_config_name(int nn_config);
int hgemm_mi355x_nn_config_by_name(const char* name);
/* out[0..7] = BM, BN, WM, WN, MI, NBUF, threads, lds_bytes (as hgemm_mi355x_config_info) */
int hgemm_mi355x_nn_config_info(int nn_config, int out[8]);
/* The plan hgemm_mi355x_nn_fp32 / _nn_fp16 run: the largest member whose tile count fills the 256 CUs, otherwise the 64 x 64 member
 * with two-pass splits so that tiles x splits reaches the chip (at most one per 64 of K, at most 32).  An analytic rule; nothing
 * is tuned per shape yet. */
int hgemm_mi355x_nn_plan(int M, int N, int K, int* nn_config, int* splits);
/* 1 when hgemm_mi355x_launch_nn runs the NN kernel itself for these dimensions and strides (pointers taken as 16-byte aligned),
 * 0 when the call falls back to the reference kernel or is refused. */
int hgemm_mi355x_nn_runs(int nn_config, int M, int N, int K, int lda, int ldb, int ldc);
/* Exactly what hgemm_mi355x_launch_nn asks for with this plan on contiguous operands: 256 KiB of counters + splits x M x N x 4 bytes
 * (0: none); hgemm_mi355x_nn_reserve_workspace makes the stream's workspace hold the planned call's. */
size_t hgemm_mi355x_nn_plan_workspace_bytes(int nn_config, int splits, int M, int N, int K);
int hgemm_mi355x_nn_reserve_workspace(int M, int N, int K, void* stream);

/* ------------------------------------------------------------------------------------------
 * TA layout (transposed A): C = A x B with A given as a_col_major ([K][M]: M contiguous) and B ROW-MAJOR ([K][N]) -- a linear
 * layer's weight gradient dW = X^T x dY, where the first operand is the activation as it is stored, [tokens][features].  With the
 * b_col_major entry points (forward) and the NN layout (input gradient) it completes the layer's three products.  The vendor
 * libraries call this form "nt"; NT means non-temporal stores throughout this library, hence "ta".  Replaces a transposed copy of A
 * (2 x M x K bytes read and written) in front of hgemm_mi355x_nn_fp32; the vendor counterpart is hgemm_rocblas_ta below.  The kernels
 * ("a" geometries, csrc/hgemm_kernel_ta.hpp) stage both operands as they lie in memory and read both MFMA operands through the
 * hardware's transposed LDS read; their table (ids 0 .. hgemm_mi355x_ta_num_configs() - 1, names a<BM>x<BN>_w<WM>x<WN>) is separate
 * from the geometry table and the NN table, which are unchanged by it.
 * Scope of the kernels: K % 64 == 0, M % 8 == 0, N % 8 == 0, lda / ldb / ldc multiples of 8, 16-byte aligned pointers, and 32-bit
 * offsets with bit 31 to spare: ((K - 1) x lda + M) x 2, ((K - 1) x ldb + N) x 2 and (BM x ldc + N) x 2 bytes each below 2 GiB.  Any
 * other call is answered by a one-output-per-thread reference kernel: HGEMM_OK, exact, slow (hgemm_mi355x_ta_runs tells).
 *
 * hgemm_mi355x_ta_fp32 / _ta_fp16: the planned calls (both accumulate in fp32); contiguous operands (lda = M, ldb = ldc = N).
 * Replace torch.matmul(x.t(), dy) / cublasGemmEx with the first operand transposed for a caller of the reference's entry points. */
int hgemm_mi355x_ta_fp32(const void* a_col_major, const void* b, void* c, int M, int N, int K, void* stream);
int hgemm_mi355x_ta_fp16(const void* a_col_major, const void* b, void* c, int M, int N, int K, void* stream);
/* The explicit call (what hgemm_mi355x_launch_nn is to the NN table).
 *   ta_config  index into the TA table
 *   splits     as hgemm_mi355x_launch_nn: the two-pass form, clamped to K / 64, 1 when no workspace is available; HGEMM_PLAN_NT_STORE is
 *              honoured, HGEMM_SPLITK_FUSED runs as the two-pass form and HGEMM_PLAN_STREAMK as the plain launch
 * lda (>= M: the row stride of a_col_major), ldb (>= N) and ldc (>= N) are in elements; a smaller stride returns HGEMM_ERR_BAD_ARG,
 * and so does an id outside the table.  Capturable like every entry point: a split plan needs its workspace beforehand
 * (hgemm_mi355x_ta_reserve_workspace), otherwise the captured call runs unsplit. */
int hgemm_mi355x_launch_ta(int ta_config, int splits, const void* a_col_major, const void* b, void* c,
                           int M, int N, int K, int lda, int ldb, int ldc, void* stream);
/* The TA table (replaces nothing in the reference: it has one kernel file per shape), with the NN functions' contracts. */
int hgemm_mi355x_ta_num_configs(void);
const char* hgemm_mi355x_ta_config_name(int ta_config);
int hgemm_mi355x_ta_config_by_name(const char* name);
int hgemm_mi355x_ta_config_info(int ta_config, int out[8]);
/* hgemm_mi355x_nn_plan's rule on the TA table: the largest member whose tile count fills the 256 CUs, otherwise the 64 x 64 member
 * with min(ceil(256 / tiles), K / 64, 32) two-pass splits. */
int hgemm_mi355x_ta_plan(int M, int N, int K, int* ta_config, int* splits);
int hgemm_mi355x_ta_runs(int ta_config, int M, int N, int K, int lda, int ldb, int ldc);
size_t hgemm_mi355x_ta_plan_workspace_bytes(int ta_config, int splits, int M, int N, int K);
int hgemm_mi355x_ta_reserve_workspace(int M, int N, int K, void* stream);
/* fp32 C, stored or accumulated ("c32"): c32 = A x B or c32 += A x B with the kernels' fp32 accumulators as they are -- the weight
 * gradient where a training step consumes it, added into an fp32 gradient buffer over the micro-batches (Megatron's main_grad, "wgrad
 * GEMM accumulate fp32").  Replaces hgemm_mi355x_ta_fp32 into an fp16 scratch (which rounds the sums to fp16: K is the token count, and
 * a sum beyond 65504 becomes inf) followed by an elementwise main_grad += float(dW16) kernel.  No fp16 value exists on the path: the result is
 * old + fl32(A x B), one fp32 add per element; the order of the sum is fixed per plan (a split plan adds its K slices in split order,
 * then the old value), so a call is deterministic.
 *   accumulate  0: c32 = A x B, the old contents of c32 are never read (they may be NaN or uninitialised); 1: c32 += A x B; any other
 *               value returns HGEMM_ERR_BAD_ARG
 * Where the rules differ from the fp16-C calls above: ldc counts fp32 elements, the kernels take ldc % 4 == 0 (not % 8) with a 16-byte
 * aligned c32, and C's reach is (BM x ldc + N) x 4 bytes below 2 GiB; the least ldc is still N.  Everything else is the TA layout's: the
 * same table and ids, the same plan (hgemm_mi355x_ta_plan: the tiles are the same), the same workspace
 * (hgemm_mi355x_ta_plan_workspace_bytes: the slabs are the same; hgemm_mi355x_ta_reserve_workspace serves both forms), the same
 * meaning of the splits word, bad strides, null pointers and ids outside the table return HGEMM_ERR_BAD_ARG, a split call without a
 * workspace runs unsplit, any call outside the kernels' scope is answered by a reference kernel (HGEMM_OK, exact, slow:
 * hgemm_mi355x_ta_c32_runs tells), and every call is capturable.  The NN and b_col_major layouts have no fp32-C form. */
/* planned, contiguous (lda = M, ldb = ldc = N) */
int hgemm_mi355x_ta_c32(const void* a_col_major, const void* b, float* c32, int M, int N, int K, int accumulate, void* stream);
/* explicit: ta_config / splits words exactly as hgemm_mi355x_launch_ta; ldc in fp32 elements */
int hgemm_mi355x_launch_ta_c32(int ta_config, int splits, const void* a_col_major, const void* b, float* c32,
                               int M, int N, int K, int lda, int ldb, int ldc, int accumulate, void* stream);
int hgemm_mi355x_ta_c32_runs(int ta_config, int M, int N, int K, int lda, int ldb, int ldc);

/* ------------------------------------------------------------------------------------------
 * bfloat16 on the NN and TA layouts ("bgemm"): the three calls above with bfloat16 operands and, for the 16-bit C, a bfloat16 result --
 * the input gradient dX = dY x W (bgemm_mi355x_nn), the weight gradient dW = X^T x dY (bgemm_mi355x_ta) and the weight gradient added
 * into an fp32 gradient buffer (bgemm_mi355x_ta_c32) for a training stack that keeps dY, X and W in bf16.  Replaces a cast of the
 * operands to fp16 in front of the hgemm_ calls (dY overflows or flushes without loss scaling) or a rocblas_gemm_ex call with bf16
 * types.  Accumulation is fp32.  The kernels are families n and a with v_mfma_f32_16x16x32_bf16 in the K loop (csrc/hgemm_kernel_nn.hpp,
 * hgemm_kernel_ta.hpp: CfgNNB / CfgTAB); the 16-bit C is the fp32 sum rounded to bf16 ONCE, to nearest even (NaN stays NaN, a sum beyond
 * the bf16 maximum becomes inf) -- in the kernel's epilogue, or in the combine of a two-pass plan, whose slabs are fp32.  The fp32 C has
 * no conversion on its path.
 * Everything else is the fp16 calls': elements are 2 bytes either way, so scope, reach and stride rules, the two tables, their ids and
 * names, the meaning of the splits word (HGEMM_PLAN_NT_STORE is honoured, HGEMM_SPLITK_FUSED runs two-pass, HGEMM_PLAN_STREAMK plain)
 * and every status are those of hgemm_mi355x_launch_nn / _launch_ta / _launch_ta_c32.  Plan, workspace size and reserve call are the
 * hgemm_mi355x_nn_* / _ta_* functions (hgemm_mi355x_nn_plan, _nn_plan_workspace_bytes, _nn_reserve_workspace, and their _ta_ twins).
 * A call outside the kernels' scope is answered by a bf16 reference kernel (HGEMM_OK, exact, slow: the _runs functions tell); every call
 * is capturable, and a captured split call without a workspace runs unsplit with status 0.  The names carry no accumulate mode: there
 * is one, fp32.
 * The b_col_major (forward) families -- hgemm_mi355x_fp32 / _fp16 / _launch -- have NO bf16 form of their own (the bf16 forward product is
 * bgemm_mi355x_tn below: kernels of its own on this path), and no existing entry point changes what it does. */
/* planned, contiguous (nn: lda = K; ta: lda = M; ldb = ldc = N) */
int bgemm_mi355x_nn(const void* a, const void* b, void* c, int M, int N, int K, void* stream);
int bgemm_mi355x_ta(const void* a_col_major, const void* b, void* c, int M, int N, int K, void* stream);
int bgemm_mi355x_ta_c32(const void* a_col_major, const void* b, float* c32, int M, int N, int K, int accumulate, void* stream);
/* explicit: config / splits words and strides exactly as hgemm_mi355x_launch_nn / _launch_ta / _launch_ta_c32 */
int bgemm_mi355x_launch_nn(int nn_config, int splits, const void* a, const void* b, void* c,
                           int M, int N, int K, int lda, int ldb, int ldc, void* stream);
int bgemm_mi355x_launch_ta(int ta_config, int splits, const void* a_col_major, const void* b, void* c,
                           int M, int N, int K, int lda, int ldb, int ldc, void* stream);
int bgemm_mi355x_launch_ta_c32(int ta_config, int splits, const void* a_col_major, const void* b, float* c32,
                               int M, int N, int K, int lda, int ldb, int ldc, int accumulate, void* stream);
/* 1 when the call runs one of the bf16 kernels, 0 when it falls back to the reference kernel or is refused (the fp16 twins' answers) */
int bgemm_mi355x_nn_runs(int nn_config, int M, int N, int K, int lda, int ldb, int ldc);
int bgemm_mi355x_ta_runs(int ta_config, int M, int N, int K, int lda, int ldb, int ldc);
int bgemm_mi355x_ta_c32_runs(int ta_config, int M, int N, int K, int lda, int ldb, int ldc);

/* ------------------------------------------------------------------------------------------
 * bfloat16 forward product ("tn"): Y = X x W^T with W stored [out][in] -- C[M,N] = A[M,K] x B[K,N], A row-major [M][lda] and B given as
 * b_col_major [N][ldb] (K contiguous), the operand form of hgemm_mi355x_fp32's b_col_major and of hgemm_rocblas_tn, with bfloat16
 * operands and a bfloat16 C.  With bgemm_mi355x_nn (dX) and bgemm_mi355x_ta / _ta_c32 (dW) a bf16 linear layer's three products.
 * Replaces a cast of X and W to fp16 in front of hgemm_mi355x_fp32 (which loses bf16's range) or a rocblas_gemm_ex call with bf16 types.
 * Accumulation is fp32; C is the fp32 sum rounded to bf16 ONCE, to nearest even -- in the kernel's epilogue, or in the combine of a
 * two-pass plan, whose slabs are fp32.  The kernels are family f (csrc/hgemm_kernel_tn.hpp): family n's ring and epilogues, both operand
 * images the classic [rows][128 B] one, v_mfma_f32_16x16x32_bf16, no transposed LDS read.
 * A third layout of the NN / TA host path, with a table of its own (four members, f64x64_w2x2 .. f128x128_w2x2: the n members' tiles,
 * ring depths and LDS bytes).  The splits word (HGEMM_PLAN_NT_STORE is honoured, HGEMM_SPLITK_FUSED runs two-pass, HGEMM_PLAN_STREAMK
 * plain), the statuses, the capture behaviour (capturable; a captured split call without a workspace runs unsplit with status 0) and
 * the planner's rule are those of hgemm_mi355x_launch_nn / _nn_plan.
 * Scope of the kernels: K % 64 == 0, N % 8 == 0 (M is free), lda / ldb / ldc multiples of 8, 16-byte aligned pointers, and
 * (BM lda + K) 2, (BN ldb + K) 2, (BM ldc + N) 2 bytes below 2 GiB.  Least strides: lda >= K, ldb >= K, ldc >= N (less: HGEMM_ERR_BAD_ARG).
 * A call outside the scope is answered by a bf16 reference kernel (HGEMM_OK, exact, slow: bgemm_mi355x_tn_runs tells).
 * The fp16 forward calls (hgemm_mi355x_fp32 / _fp16 / _launch, the geometry table, hgemm_mi355x_plan) are unchanged, and there is no
 * fp16 "tn" call on this path: fp16 callers have those. */
/* planned, contiguous (lda = ldb = K, ldc = N) */
int bgemm_mi355x_tn(const void* a, const void* b_col_major, void* c, int M, int N, int K, void* stream);
int bgemm_mi355x_launch_tn(int tn_config, int splits, const void* a, const void* b_col_major, void* c,
                           int M, int N, int K, int lda, int ldb, int ldc, void* stream);
/* 1 when the call runs one of the family's kernels, 0 when it falls back to the reference kernel or is refused */
int bgemm_mi355x_tn_runs(int tn_config, int M, int N, int K, int lda, int ldb, int ldc);
int bgemm_mi355x_tn_num_configs(void);
const char* bgemm_mi355x_tn_config_name(int tn_config);
int bgemm_mi355x_tn_config_by_name(const char* name);
int bgemm_mi355x_tn_config_info(int tn_config, int out[8]);   /* as hgemm_mi355x_nn_config_info */
int bgemm_mi355x_tn_plan(int M, int N, int K, int* tn_config, int* splits);
size_t bgemm_mi355x_tn_plan_workspace_bytes(int tn_config, int splits, int M, int N, int K);
int bgemm_mi355x_tn_reserve_workspace(int M, int N, int K, void* stream);

/* ------------------------------------------------------------------------------------------
 * Forward product with a fused bias: Y = X x W^T + b, a linear layer's whole forward in one call.  Operands, layout, strides and scope
 * are bgemm_mi355x_tn's; `bias` is a bfloat16 device vector of N contiguous elements, read-only, owned by the caller like a and
 * b_col_major (it must stay valid until the call has run on `stream`).
 * Replaces bgemm_mi355x_tn followed by an element-wise add -- a second pass that reads and writes all of Y again (4 M N bytes for a
 * 2 N byte vector) and rounds to bf16 a second time -- or a vendor GEMM with a bias epilogue (hipblasLt's HIPBLASLT_EPILOGUE_BIAS).
 * Semantics, exactly:  C[m][n] = bf16( fl32( S[m][n] + float(bias[n]) ) ).
 *   - S is the finished fp32 sum of the product: the accumulator behind the K walk of a plain launch, or the slabs of a two-pass plan
 *     added in split order.
 *   - The bias is added last, as ONE fp32 add to the finished sum: it is not the accumulators' initial value and it is not added into
 *     a slab.
 *   - The result is rounded once, to nearest even.
 * No activation and no fp16 form.  bias == NULL: HGEMM_ERR_BAD_ARG (a caller without a bias has bgemm_mi355x_tn).
 * The kernels (family f's fused-bias epilogue) also want `bias` 16-byte aligned; any other call is answered by the reference kernel
 * (HGEMM_OK, exact, slow).  The table, ids, names, plan, workspace size and reserve call are bgemm_mi355x_tn_*'s -- the tiles, cuts and
 * slabs of a bias call are those of the bgemm_mi355x_launch_tn call with the same arguments -- and so are the splits word, the statuses
 * and the capture behaviour. */
/* planned, contiguous (lda = ldb = K, ldc = N) */
int bgemm_mi355x_tn_bias(const void* a, const void* b_col_major, const void* bias, void* c, int M, int N, int K, void* stream);
int bgemm_mi355x_launch_tn_bias(int tn_config, int splits, const void* a, const void* b_col_major, const void* bias, void* c,
                                int M, int N, int K, int lda, int ldb, int ldc, void* stream);
/* 1 when the call (with an aligned bias) runs one of the family's kernels: equal to bgemm_mi355x_tn_runs */
int bgemm_mi355x_tn_bias_runs(int tn_config, int M, int N, int K, int lda, int ldb, int ldc);

/* ------------------------------------------------------------------------------------------
 * Forward product with a fused bias AND activation: Y = act(X x W^T + b), the first half of a transformer MLP in one call.  Operands,
 * `bias`, layout, strides and scope are bgemm_mi355x_tn_bias's.
 * Replaces bgemm_mi355x_tn_bias followed by an element-wise activation kernel -- a second launch and a second pass that reads and
 * writes all of Y again (4 M N bytes), with the activation applied to a value already rounded to bf16 -- or a vendor GEMM with a
 * bias+ReLU / bias+GELU epilogue.
 * Semantics, exactly:  z[m][n] = fl32( S[m][n] + float(bias[n]) )   (bgemm_mi355x_tn_bias's value before its rounding)
 *                      C[m][n] = bf16_rne( act32( z[m][n] ) )
 *   - S is the finished fp32 sum: the accumulator of a plain launch, or the slabs of a two-pass plan added in split order; the bias
 *     is added last.
 *   - The activation is applied to the unrounded sum z, in fp32.  It is never applied to a slab.  The result is rounded once.
 *   - `act` is one of
 *       HGEMM_ACT_RELU       y = z if z > 0 or z is NaN, otherwise +0.0f.  -0, -inf and every negative give +0, NaN stays NaN, +inf
 *                            stays +inf.  An exact function: C is defined bit for bit.
 *       HGEMM_ACT_GELU       y = 0.5 z (1 + erf(z / sqrt 2)), the erf form (torch's default).
 *       HGEMM_ACT_GELU_TANH  y = 0.5 z (1 + tanh(sqrt(2 / pi) (z + 0.044715 z^3))), the GPT-2 / BERT form, evaluated as the
 *                            algebraically equal z / (1 + exp(-2u)).  A large negative finite z (z^3 overflows) gives -0, a large
 *                            positive z gives z.
 *     Both GELUs: NaN gives NaN, +inf gives +inf, -inf gives NaN (the formulas' own 0 x inf, as torch has it), z = +-0 gives a zero.
 *   - The GELU bar: with y* the activation of the exact z evaluated in fp64, every finite element satisfies
 *       |C - y*| <= 1/2 ulp_bf16(y*) + 2^-19 |z|
 *     (the second term covers the fp32 evaluation of 1 + erf / 1 + tanh, 16 and 5 ulp in the device math library, times |z| / 2; it
 *     matters only in the negative tail).  The plain, split and reference forms of one call share one activation text.
 * act == 0 or any other value: HGEMM_ERR_BAD_ARG (a caller with no activation has bgemm_mi355x_tn_bias).  bias == NULL:
 * HGEMM_ERR_BAD_ARG -- a layer without a bias passes a zero vector.  No fp16 form, no other layout; HGEMM_ACT_SILU is refused here --
 * SiLU and the gated forms (SwiGLU, GeGLU, ReGLU) are bgemm_mi355x_tn_gated, below.
 * The table, ids, names, plan, workspace size and reserve call are bgemm_mi355x_tn_*'s: the tiles, cuts, slabs, splits word, statuses
 * and capture behaviour of a call are those of the bgemm_mi355x_launch_tn call with the same arguments. */
#define HGEMM_ACT_RELU 1
#define HGEMM_ACT_GELU 2
#define HGEMM_ACT_GELU_TANH 3
/* planned, contiguous (lda = ldb = K, ldc = N) */
int bgemm_mi355x_tn_bias_act(const void* a, const void* b_col_major, const void* bias, void* c, int M, int N, int K, int act, void* stream);
int bgemm_mi355x_launch_tn_bias_act(int tn_config, int splits, const void* a, const void* b_col_major, const void* bias, void* c,
                                    int M, int N, int K, int lda, int ldb, int ldc, int act, void* stream);
/* 1 when the call (with an aligned bias) runs one of the family's kernels: equal to bgemm_mi355x_tn_runs */
int bgemm_mi355x_tn_bias_act_runs(int tn_config, int M, int N, int K, int lda, int ldb, int ldc);

/* ------------------------------------------------------------------------------------------
 * Gated forward product: H = act(X x Wg^T + bg) (.) (X x Wu^T + bu), the first half of a SwiGLU / GeGLU / ReGLU MLP (Llama, Mistral,
 * Qwen, Gemma, PaLM) in one call.  a = X [M][lda]; wg_col_major and wu_col_major are each [N][ldb] with K contiguous, N the OUTPUT width,
 * one ldb for both; a fused [2N][K] gate_up weight is passed as wu = wg + N ldb, and wg == wu is allowed (both are only read).  c = H,
 * bf16 [M][ldc], overlapping no input.
 * Replaces two bgemm_mi355x_tn_bias* calls, each rounding to bf16, and an element-wise kernel -- or one bgemm_mi355x_tn on the stacked
 * weight and an element-wise kernel that reads 2 M 2N bytes back and writes M N 2 more; either way the activation sees a rounded value.
 * Semantics, exactly:  g[m][n] = fl32( Sg[m][n] + float(bias_g[n]) )      Sg = X x Wg^T, the finished fp32 sum
 *                      u[m][n] = fl32( Su[m][n] + float(bias_u[n]) )      Su = X x Wu^T
 *                      C[m][n] = bf16_rne( fl32( act32(g[m][n]) x u[m][n] ) )
 *   - A finished sum is the accumulator of a plain launch, or the slabs of a two-pass plan added in split order.  Bias, activation and
 *     gate are applied once, to finished sums, never to a slab.  One bf16 rounding.
 *   - `act` is HGEMM_ACT_RELU, HGEMM_ACT_GELU, HGEMM_ACT_GELU_TANH (as above) or
 *       HGEMM_ACT_SILU       y = z / (1 + exp(-z)).  NaN gives NaN, +inf gives +inf, -inf gives NaN (inf / inf), a large negative finite
 *                            z gives -0, z = +-0 gives a zero.
 *     Any other value: HGEMM_ERR_BAD_ARG.  HGEMM_ACT_SILU is accepted by the gated calls alone.
 *   - bias_g == NULL or bias_u == NULL (each on its own) means a vector of +0.0: the result is that of a zero-filled vector, bit for bit.
 *   - The bar: with y* = act*(g) u in fp64 on the exact g and u, every finite element satisfies
 *       |C - y*| <= 1/2 ulp_bf16(y*) + 2^-19 |g| |u| + 2^-23 |y*|
 *     (the activation's fp32 evaluation, the fp32 product, the one rounding).  With HGEMM_ACT_RELU C is defined bit for bit.
 * The call does the work of a TN product of width 2N: the planned call takes its member and splits from bgemm_mi355x_tn_plan(M, 2N, K);
 * workspace size and reserve are bgemm_mi355x_tn_plan_workspace_bytes(cfg, splits, M, 2N, K) and bgemm_mi355x_tn_reserve_workspace(M, 2N,
 * K, stream).  Ids, names, the splits word, HGEMM_PLAN_NT_STORE, statuses, the capture rules and the no-workspace fallback during capture
 * (unsplit, HGEMM_OK, nothing allocated) are bgemm_mi355x_launch_tn's.  A member's tile is BM rows by BN / 2 output columns.
 * Scope of the kernels: K % 64 == 0, N % 8 == 0, lda / ldb / ldc multiples of 8, a, both weights, c and any non-NULL bias 16-byte
 * aligned, (BM lda + K) 2, (BN / 2 ldb + K) 2 for each weight and (BM ldc + N) 2 bytes below 2 GiB.  Everything else is answered by the
 * reference kernel (status 0, the same semantics).  NULL a, wg, wu or c, N >= 2^30: HGEMM_ERR_BAD_ARG.  No fp16 form, no other layout. */
#define HGEMM_ACT_SILU 4   /* the gated calls only: bgemm_mi355x_tn_gated and its input gradient, bgemm_mi355x_nn_dgated */
/* planned, contiguous (lda = ldb = K, ldc = N) */
int bgemm_mi355x_tn_gated(const void* a, const void* wg_col_major, const void* wu_col_major, const void* bias_g, const void* bias_u, void* c,
                          int M, int N, int K, int act, void* stream);
int bgemm_mi355x_launch_tn_gated(int tn_config, int splits, const void* a, const void* wg_col_major, const void* wu_col_major,
                                 const void* bias_g, const void* bias_u, void* c, int M, int N, int K, int lda, int ldb, int ldc, int act,
                                 void* stream);
/* 1 when the call (with aligned operands) runs one of the family's kernels */
int bgemm_mi355x_tn_gated_runs(int tn_config, int M, int N, int K, int lda, int ldb, int ldc);

/* ------------------------------------------------------------------------------------------
 * Training forward that also saves the pre-activation: Y = act(X x W^T + b) AND Z = X x W^T + b, both bf16, in one call.  Operands,
 * `bias`, `act`, layout, strides and scope are bgemm_mi355x_tn_bias_act's; `z_out` is a second bf16 output [M][ldz].
 * Replaces bgemm_mi355x_tn_bias followed by an element-wise activation kernel, or both GEMMs: the backward pass through the activation
 * needs z, and the rounded Y does not determine it.  The vendor libraries' GELU_AUX_BIAS epilogue.
 * Semantics, exactly:  z[m][n]     = fl32( S[m][n] + float(bias[n]) )
 *                      z_out[m][n] = bf16_rne( z[m][n] )
 *                      C[m][n]     = bf16_rne( act32( z[m][n] ) )
 *   - The activation is applied to the UNROUNDED z, as in bgemm_mi355x_tn_bias_act; both outputs are rounded once.
 *   - Two identities, bit for bit, for the same arguments and plan: C is the C of bgemm_mi355x_launch_tn_bias_act, and z_out is the C
 *     of bgemm_mi355x_launch_tn_bias.  The plain, two-pass (the combine writes both outputs; no slab is touched) and reference forms
 *     all hold them.  HGEMM_PLAN_NT_STORE applies to both outputs.
 * z_out has C's rules: ldz >= N (less: HGEMM_ERR_BAD_ARG); 16-byte aligned, ldz % 8 == 0 and (BM ldz + N) 2 bytes below 2 GiB, or the
 * reference kernel answers.  z_out == NULL and z_out == c: HGEMM_ERR_BAD_ARG; z_out and C must not overlap.  act and bias: as in
 * bgemm_mi355x_tn_bias_act.  No fp16 form, no other layout.
 * The table, ids, names, plan, workspace size and reserve call are bgemm_mi355x_tn_*'s: the tiles, cuts and slabs of a call are those
 * of the bgemm_mi355x_launch_tn call with the same arguments. */
/* planned, contiguous (lda = ldb = K, ldc = ldz = N) */
int bgemm_mi355x_tn_bias_act_aux(const void* a, const void* b_col_major, const void* bias, void* c, void* z_out, int M, int N, int K, int act,
                                 void* stream);
int bgemm_mi355x_launch_tn_bias_act_aux(int tn_config, int splits, const void* a, const void* b_col_major, const void* bias, void* c,
                                        void* z_out, int M, int N, int K, int lda, int ldb, int ldc, int ldz, int act, void* stream);
/* 1 when the call (with aligned bias and z_out) runs one of the family's kernels: bgemm_mi355x_tn_runs when ldz >= N, ldz % 8 == 0 and
 * z_out is within reach, otherwise 0 (ldz < N, which the launch refuses, included).  No activation changes the answer. */
int bgemm_mi355x_tn_bias_act_aux_runs(int tn_config, int M, int N, int K, int lda, int ldb, int ldc, int ldz);

/* ------------------------------------------------------------------------------------------
 * Input gradient through the activation: dZ = (dY x W) (.) act'(Z), the backward of the layer above in one call.  a = dY [M][K],
 * b = W [K][N] row-major (bgemm_mi355x_nn's operand form), `z` = the saved bf16 pre-activation [M][ldz] (read-only: the z_out of
 * bgemm_mi355x_tn_bias_act_aux), c = dZ [M][ldc], bf16.
 * Replaces bgemm_mi355x_nn followed by an element-wise kernel that reads dH and Z and writes dH (.) act'(Z): one more launch, 6 M N
 * more bytes and a second rounding (dH rounded to bf16 before the multiply).  The vendor libraries' DGELU epilogue.
 * Semantics, exactly:  zf      = float( z[m][n] )                       (exact: a bf16 value is an fp32 value)
 *                      C[m][n] = bf16_rne( fl32( S[m][n] x dact32(zf) ) )
 *   - S is the finished fp32 sum: the accumulator of a plain launch, or the slabs of a two-pass plan added in split order.  The
 *     multiplication is ONE fp32 multiply on the finished sum, never on a slab; the result is rounded once; no bf16 dH exists.
 *   - `act` is one of
 *       HGEMM_ACT_RELU       C = (zf <= 0) ? +0.0f : bf16(S): a select, not a multiply.  -0 and -inf give +0, whatever S holds; a NaN z
 *                            passes S (torch's threshold_backward).  Defined bit for bit.
 *       HGEMM_ACT_GELU       g = 1/2 (1 + erf(z / sqrt 2)) + z exp(-z^2 / 2) / sqrt(2 pi)
 *       HGEMM_ACT_GELU_TANH  g = s + z s (1 - s) 2u', s = 1 / (1 + exp(-2u)), u = sqrt(2 / pi) (z + 0.044715 z^3),
 *                            u' = sqrt(2 / pi) (1 + 3 x 0.044715 z^2): the derivative of bgemm_mi355x_tn_bias_act's own sigmoid form.
 *     Both GELUs: g is finite for every finite z -- z is clamped to [-16, 16] first, behind which nothing overflows and outside which
 *     g is within 2^-180 of its limit; every z >= 16, +inf included, gives exactly 1, every z <= -16, -inf included, gives +0 (so
 *     C = +-0 or, for a non-finite S, NaN).  A NaN z gives NaN.
 *   - The GELU bar: with g* the derivative of the given z evaluated in fp64, every element with a finite S satisfies
 *       |C - S g*(zf)| <= 1/2 ulp_bf16(S g*) + 2^-19 |S|.
 *     2^-19 is derived, not measured (csrc/hgemm_act.hpp has the full count): the device math library's erff within 16 ulp (32 x 2^-24)
 *     and expf within 1 ulp, a correctly rounded division, every fp32 product, sum and fmaf within 2^-24 relatively, propagated
 *     through the formulas with |g| <= 1.13, and the multiply S g itself, give 21.9 x 2^-24 (erf form) and 15.6 x 2^-24 (tanh form),
 *     both below 32 x 2^-24 = 2^-19.  The plain, split and reference forms of one call share one derivative text.
 * z has C's rules: ldz >= N (less: HGEMM_ERR_BAD_ARG); 16-byte aligned, ldz % 8 == 0 and (BM ldz + N) 2 bytes below 2 GiB, or the
 * reference kernel answers.  M is free: a z (and C) of 4 GiB and more is in scope.  The kernels read z through a range that ends at its
 * last valid element (M - 1, N - 1), or 4 GiB behind a tile's first row where z goes on further than that: no byte behind the last
 * element is touched and pad columns do not matter.  z == NULL, z == c and any act outside 1..3: HGEMM_ERR_BAD_ARG.
 * Out of scope: no fp16 form; no TA / TN form; no bias gradient -- this call writes dZ alone; bgemm_mi355x_nn_dact_dbias below is the
 * same call with the column sum of dZ, reduced across workgroups in a fixed order.
 * The table, ids, names, plan, workspace size and reserve call are hgemm_mi355x_nn_*'s: the tiles, cuts and slabs of a call are those
 * of the bgemm_mi355x_launch_nn call with the same arguments. */
/* planned, contiguous (lda = K, ldb = ldc = ldz = N) */
int bgemm_mi355x_nn_dact(const void* a, const void* b, const void* z, void* c, int M, int N, int K, int act, void* stream);
int bgemm_mi355x_launch_nn_dact(int nn_config, int splits, const void* a, const void* b, const void* z, void* c, int M, int N, int K,
                                int lda, int ldb, int ldc, int ldz, int act, void* stream);
/* 1 when the call (with an aligned z) runs one of the family's kernels: hgemm_mi355x_nn_runs when ldz >= N, ldz % 8 == 0 and z is
 * within reach, otherwise 0 (ldz < N, which the launch refuses, included).  No activation changes the answer. */
int bgemm_mi355x_nn_dact_runs(int nn_config, int M, int N, int K, int lda, int ldb, int ldc, int ldz);

/* ------------------------------------------------------------------------------------------
 * The same with the bias gradient: dZ as above and db = the column sum of dZ, in one call.  Replaces a framework reduction over dZ behind
 * bgemm_mi355x_nn_dact: one more launch, 2 M N more bytes, and an order of summation that is not this library's.
 * Semantics, exactly:
 *   - C[m][n] is the C of bgemm_mi355x_launch_nn_dact for the same arguments and plan, bit for bit.
 *   - s[n] = sum over m < M of float( C[m][n] ): the sum of the ROUNDED bf16 values the call stores -- db matches the dZ the dW GEMM
 *     (bgemm_mi355x_ta_c32) will read --, taken in fp32.  The order is fixed for a given (plan, strides, alignment, workspace present or
 *     not): two identical calls give identical bits, and HGEMM_PLAN_NT_STORE does not change the bits.  A row at or past M counts 0.
 *   - accumulate == 0: db32[n] = s[n]; the old contents are never read and may be NaN.
 *     accumulate == 1: db32[n] = fl32( old + s[n] ), one fp32 add, as in hgemm_mi355x_ta_c32.
 *     Any other value: HGEMM_ERR_BAD_ARG.
 *   - db32 holds N contiguous floats; db32 == NULL: HGEMM_ERR_BAD_ARG; 4-byte alignment is enough; nothing behind db32[N-1] is written.
 *   - The bar of the sum: |s[n] - sum_m C[m][n]| <= gamma_{M-1} sum_m |C[m][n]|, gamma_k = k u / (1 - k u), u = 2^-24: the standard
 *     bound of an M-term fp32 sum in any order, derived, not measured (csrc/hgemm_dbias.hpp).  Where every partial sum is exact in fp32
 *     (integer data), s is exact.
 * Everything else is bgemm_mi355x_nn_dact's: act, z, ldz, strides, scope, statuses, table, plan and refusals, the reference form, M free.
 * How a call runs (the order of the sum follows from it):
 *   - plain plan: the member's kernel sums its finished, rounded tile by column in its epilogue -- per lane over its fragments, a fixed
 *     butterfly over the 16 rows of a fragment, the wave rows through LDS in order -- and writes tiles_m x N fp32 partials to the stream's
 *     workspace; a second small kernel adds them over tile_m = 0 .. tiles_m - 1 in that order and writes or adds into db32.
 *   - two-pass plan: the K slices and the dact combine unchanged, then bgemm_mi355x_colsum_c32's sum of the C just written.
 *   - reference form (misaligned pointer, ldz % 8 != 0, ...): the reference dact kernel, then the direct column sum of C.
 *   - no workspace (a capturing stream without a reserve, a lent buffer too small): still HGEMM_OK and a correct db -- the dact kernel of
 *     bgemm_mi355x_nn_dact, unsplit, then the direct column sum, which needs none.  Nothing is allocated during capture.
 * Workspace: counters + tiles_m x N x 4 bytes (plain), + the slabs and the sum's partials (two-pass); _plan_workspace_bytes reports what
 * a launch with that plan on contiguous operands asks for, _reserve_workspace sizes the stream's workspace for the planned call.
 * Out of scope: no fp16 form, no other layout, no bf16 db, no db inside the dW kernel or the two-pass combine. */
/* planned, contiguous (lda = K, ldb = ldc = ldz = N) */
int bgemm_mi355x_nn_dact_dbias(const void* a, const void* b, const void* z, void* c, float* db32, int M, int N, int K, int act,
                               int accumulate, void* stream);
int bgemm_mi355x_launch_nn_dact_dbias(int nn_config, int splits, const void* a, const void* b, const void* z, void* c, float* db32, int M,
                                      int N, int K, int lda, int ldb, int ldc, int ldz, int act, int accumulate, void* stream);
/* bgemm_mi355x_nn_dact_runs: the bias gradient changes no scope */
int bgemm_mi355x_nn_dact_dbias_runs(int nn_config, int M, int N, int K, int lda, int ldb, int ldc, int ldz);
size_t bgemm_mi355x_nn_dact_dbias_plan_workspace_bytes(int nn_config, int splits, int M, int N, int K);
int bgemm_mi355x_nn_dact_dbias_reserve_workspace(int M, int N, int K, void* stream);

/* The column sum on its own: out32[n] (+)= sum over m < M of float( x[m][n] ), x a bf16 matrix [M][ldx].  The bias gradient of a layer
 * without an activation (db = sum over m of dY), and what the call above falls back to.  Any M, N >= 1; ldx >= N (less:
 * HGEMM_ERR_BAD_ARG); x == NULL, out32 == NULL and accumulate outside 0 / 1: HGEMM_ERR_BAD_ARG.  accumulate as above; out32 holds N floats.
 * fp32 throughout, deterministic per (M, N, ldx, alignment, workspace present or not), the bar above.  M > 256 and a workspace: row blocks
 * of 256 rows to fp32 partials in the stream's workspace -- 16-byte loads where ldx % 8 == 0 and x is 16-byte aligned (the last N % 8 columns
 * by 2-byte loads), 2-byte loads otherwise; the same adds in the same order either way --, then the finish kernel of the call above.  Otherwise, and without a workspace: one thread per column walks the M
 * rows in order. */
int bgemm_mi355x_colsum_c32(const void* x, float* out32, int M, int N, int ldx, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------
 * Input gradient of the gated MLP (SwiGLU, GeGLU, ReGLU): with H = act(G) (.) U the layer bgemm_mi355x_tn_gated computes and dH = dY x Wd,
 *     dU = act(G) (.) dH          dG = dH (.) U (.) act'(G)
 * in one call.  a = dY [M][lda] (K = the model width), b = Wd [K][ldb] row-major (N = the MLP's inner width): bgemm_mi355x_nn's operands.
 * `g` and `u` are the saved bf16 pre-activations, each [M][ldz], read-only, one ldz for both; `dg` and `du` the bf16 outputs, each
 * [M][ldc], one ldc for both.  The saved [g|u] is the [M][2N] output of ONE bgemm_mi355x_tn_bias (or bgemm_mi355x_tn) call on the fused
 * [2N][K] gate_up weight: pass u = g + N with ldz >= 2N (g == u is allowed).  A fused [M][2N] gradient is du = dg + N with ldc >= 2N; the
 * next two products are then existing calls -- dX = [dG|dU] x [Wg;Wu] is bgemm_mi355x_nn with K = 2N, dW_gate_up += X^T x [dG|dU] is
 * bgemm_mi355x_ta_c32 with N = 2N -- and the bias gradients are bgemm_mi355x_colsum_c32 over the [M][2N] result.
 * Replaces bgemm_mi355x_nn followed by an element-wise kernel that reads dH, g, u and writes dG, dU: one more launch, 10 M N more bytes,
 * and dH rounded to bf16 before it meets the gate.
 * Semantics, exactly:  gf = float( g[m][n] ), uf = float( u[m][n] )         (exact)
 *                      du[m][n] = bf16_rne( fl32( act32(gf) x S ) )
 *                      dg[m][n] = bf16_rne( dact_mul<act>( fl32( S x uf ), gf ) )
 *   - S is the finished fp32 sum: the accumulator of a plain launch, or the slabs of a two-pass plan added in split order.  Nothing is
 *     applied to a slab, each output is rounded once, no bf16 dH exists.
 *   - act32 is bgemm_mi355x_tn_gated's activation; dact_mul is bgemm_mi355x_nn_dact's: for HGEMM_ACT_RELU the select gf <= 0 ? +0 : value,
 *     otherwise one fp32 multiply by the derivative.  `act` is HGEMM_ACT_RELU, _GELU, _GELU_TANH or _SILU (SiLU stays refused by the dact
 *     calls).  SiLU's derivative is s + z s (1 - s), s = 1 / (1 + exp(-z)), evaluated on |z| clamped to 128: every z >= 128, +inf
 *     included, gives exactly 1, every z <= -128, -inf included, +0; NaN gives NaN.
 *   - The bars, fp64 values on the given S, gf, uf, for every element with a finite S (csrc/hgemm_dgated.hpp and hgemm_act.hpp derive them):
 *       |du - act*(gf) S|      <= 1/2 ulp_bf16(.) + 2^-19 |gf| |S| + 2^-23 |.|
 *       |dg - S uf act'*(gf)|  <= 1/2 ulp_bf16(.) + 2^-19 |S uf|
 *     ReLU is defined bit for bit for both outputs.
 * Scope is bgemm_mi355x_nn_dact's with z replaced by two inputs and C by two outputs: K % 64 == 0, N % 8 == 0, every stride a multiple of
 * 8, all six pointers 16-byte aligned, (BM ldc + N) 2 and (BM ldz + N) 2 bytes below 2 GiB, M free; anything else is answered by the
 * reference kernel (status 0, the same semantics).  g and u are each read through a range that ends at that matrix's last valid element.
 * Refused with HGEMM_ERR_BAD_ARG: any NULL of the six pointers, dg == du, an output equal to g or u (no in-place form), ldz < N, ldc < N, a
 * bad id, any other act.
 * The table, ids, names, plan (hgemm_mi355x_nn_plan(M, N, K)), workspace size and reserve call are hgemm_mi355x_nn_*'s, the splits word
 * and HGEMM_PLAN_NT_STORE (both outputs) bgemm_mi355x_launch_nn_dact's; a captured split call without a workspace runs unsplit, status 0,
 * and allocates nothing.
 * The forward that writes H and [g|u] in one call is bgemm_mi355x_tn_gated_aux, below.
 * Out of scope: a bias gradient inside this call, in-place operation, fp16. */
/* planned, contiguous (lda = K, ldb = ldz = ldc = N) */
int bgemm_mi355x_nn_dgated(const void* a, const void* b, const void* g, const void* u, void* dg, void* du, int M, int N, int K, int act,
                           void* stream);
int bgemm_mi355x_launch_nn_dgated(int nn_config, int splits, const void* a, const void* b, const void* g, const void* u, void* dg, void* du,
                                  int M, int N, int K, int lda, int ldb, int ldz, int ldc, int act, void* stream);
/* bgemm_mi355x_nn_dact_runs(nn_config, M, N, K, lda, ldb, ldc, ldz): the second input and output change no scope (note the order of the
 * last two arguments here) */
int bgemm_mi355x_nn_dgated_runs(int nn_config, int M, int N, int K, int lda, int ldb, int ldz, int ldc);

/* ------------------------------------------------------------------------------------------
 * Training form of the gated forward product: bgemm_mi355x_tn_gated that also saves the bf16 pre-activations g and u, the two matrices
 * bgemm_mi355x_nn_dgated reads.  Operands, `act`, the NULL-bias rule, layout, strides, table, ids, names, plan (bgemm_mi355x_tn_plan(M, 2N, K)),
 * workspace size, reserve call, splits word and capture behaviour are bgemm_mi355x_tn_gated's.  `g_out` and `u_out` are two more bf16
 * outputs, each [M][ldz], one ldz for both.
 * Fused buffer: u_out = g_out + N with ldz >= 2N is the [M][2N] matrix g|u that bgemm_mi355x_nn_dgated takes as it is (u = g + N, its ldz =
 * this call's).  One gated MLP layer's forward and backward are then this library's calls on their fused buffers: this call writes H and
 * g|u, bgemm_mi355x_nn_dgated writes dg|du, bgemm_mi355x_nn at K = 2N gives dX, bgemm_mi355x_ta_c32 at N = 2N gives dW and
 * bgemm_mi355x_colsum_c32 gives db.
 * Semantics, exactly, with g and u the fp32 values of bgemm_mi355x_tn_gated (finished sum + float(bias), one fp32 add each):
 *     g_out[m][n] = bf16_rne( g[m][n] )     u_out[m][n] = bf16_rne( u[m][n] )     C[m][n] = bf16_rne( fl32( act32(g[m][n]) x u[m][n] ) )
 *   - The activation and the gate see the UNROUNDED g and u.  Each of the three outputs is rounded once.  Nothing is applied to a slab: in
 *     a two-pass plan the combine writes all three outputs.  HGEMM_PLAN_NT_STORE applies to all three outputs.
 *   - C keeps bgemm_mi355x_tn_gated's bar (ReLU bit for bit); g_out and u_out are defined bit for bit for every activation.
 * Identities, for the same tn_config, splits word and arguments:
 *   - C is the C of bgemm_mi355x_launch_tn_gated, bit for bit.
 *   - g_out is the C of bgemm_mi355x_launch_tn_bias(tn_config, splits, a, wg, bias_g, ...) at (M, N, K), bit for bit on arbitrary operands,
 *     and u_out the same with wu and bias_u (a NULL bias: a zero-filled vector): each accumulator walks K in the same order whatever the
 *     tile's width.  This holds for every unsplit launch (plain and NT), and for a split launch wherever both calls resolve to the same K
 *     cuts -- they do whenever both run their kernels, the cuts depend on K and the splits word alone.
 * Scope: bgemm_mi355x_tn_gated's, and g_out and u_out have C's rules: 16-byte aligned, ldz % 8 == 0, (BM ldz + N) 2 bytes below 2 GiB;
 * anything else is answered by the reference kernel (status 0, the same semantics).
 * Refused with HGEMM_ERR_BAD_ARG: everything bgemm_mi355x_tn_gated refuses, a NULL g_out or u_out, g_out == u_out, either of them equal
 * to c, ldz < N.  Overlap of the three outputs with each other or with an input is the caller's error.
 * The two ends of the chain that meet the residual stream are bgemm_mi355x_tn_bias_add (X_out = X_in + H x Wd^T + b) and
 * bgemm_mi355x_nn_add at K = 2N (dX = [dG|dU] x [Wg;Wu] + dX_out), below.
 * Out of scope: fp16, a bias gradient, more than two saved matrices. */
/* planned, contiguous (lda = ldb = K, ldc = ldz = N) */
int bgemm_mi355x_tn_gated_aux(const void* a, const void* wg_col_major, const void* wu_col_major, const void* bias_g, const void* bias_u, void* c,
                              void* g_out, void* u_out, int M, int N, int K, int act, void* stream);
int bgemm_mi355x_launch_tn_gated_aux(int tn_config, int splits, const void* a, const void* wg_col_major, const void* wu_col_major,
                                     const void* bias_g, const void* bias_u, void* c, void* g_out, void* u_out, int M, int N, int K, int lda,
                                     int ldb, int ldc, int ldz, int act, void* stream);
/* bgemm_mi355x_tn_gated_runs with g_out's and u_out's conditions added; 0 for ldz < N */
int bgemm_mi355x_tn_gated_aux_runs(int tn_config, int M, int N, int K, int lda, int ldb, int ldc, int ldz);

/* ------------------------------------------------------------------------------------------
 * Forward product with a fused bias and residual add: X_out = X_in + (H x Wd^T + b), a down projection (or an attention output
 * projection) written straight into the residual stream.  Operands, layout, strides and scope are bgemm_mi355x_tn_bias's; `r` = X_in is a
 * bf16 matrix [M][ldr], read-only.  The vendor libraries' beta = 1.
 * Replaces bgemm_mi355x_tn_bias followed by an element-wise add: a second launch, 6 M N more bytes and a second bf16 rounding.
 * Semantics, exactly:  z       = fl32( S[m][n] + float(bias[n]) )        (bgemm_mi355x_tn_bias's value before its rounding)
 *                      C[m][n] = bf16_rne( fl32( z + float(r[m][n]) ) )
 *   - S is the finished fp32 sum: the accumulator of a plain launch, or the slabs of a two-pass plan added in split order.
 *   - Two fp32 adds IN THIS ORDER, then one rounding.  Nothing is added to a slab.
 *   - bias == NULL means a vector of +0.0, bit for bit (the gated calls' rule): a layer without a bias has no other call to fall back on.
 *   - Identity with bgemm_mi355x_launch_tn_bias (same tn_config, splits word and arguments): for an r of +0.0, C equals that call's C
 *     wherever z is not -0; for z = -0 this call gives +0 (-0 + +0 = +0) where that call gives -0.
 * In place: r == c with ldr == ldc is allowed and defined -- each C[m][n] is computed from the OLD r[m][n] (x += f(h)), in the kernels, in
 * the two-pass combine and in the reference kernel alike; pad columns of c stay untouched.  r == c with ldr != ldc: HGEMM_ERR_BAD_ARG.  Any
 * other overlap of r and c, and an overlap of c with a, b_col_major or bias, is the caller's error, as in bgemm_mi355x_tn_bias.
 * r has bgemm_mi355x_nn_dact's rules for z: ldr >= N (less: HGEMM_ERR_BAD_ARG); 16-byte aligned, ldr % 8 == 0 and (BM ldr + N) 2 bytes below
 * 2 GiB, or the reference kernel answers (status 0, the same semantics).  The kernels read r through a range that ends at its last valid
 * element (M - 1, N - 1): no byte behind it is touched and pad columns do not matter.
 * Refused with HGEMM_ERR_BAD_ARG: a NULL a, b_col_major, r or c, bad strides, an id outside the table.
 * The table, ids, names, plan, workspace size and reserve call are bgemm_mi355x_tn_*'s: the tiles, cuts and slabs of a call are those of the
 * bgemm_mi355x_launch_tn_bias call with the same arguments, and so are the splits word, HGEMM_PLAN_NT_STORE, the statuses and the capture
 * behaviour (a captured split call without a workspace runs unsplit, status 0, and allocates nothing).
 * Out of scope: beta other than 1, an fp32 or fp16 r, an activation behind the add, fp16, the TA layout (its fp32 form accumulates), the
 * gated calls. */
/* planned, contiguous (lda = ldb = K, ldc = ldr = N) */
int bgemm_mi355x_tn_bias_add(const void* a, const void* b_col_major, const void* bias, const void* r, void* c, int M, int N, int K, void* stream);
int bgemm_mi355x_launch_tn_bias_add(int tn_config, int splits, const void* a, const void* b_col_major, const void* bias, const void* r, void* c,
                                    int M, int N, int K, int lda, int ldb, int ldc, int ldr, void* stream);
/* 1 when the call (with aligned pointers) runs one of the family's kernels: bgemm_mi355x_tn_bias_runs with r's conditions added; 0 for
 * ldr < N */
int bgemm_mi355x_tn_bias_add_runs(int tn_config, int M, int N, int K, int lda, int ldb, int ldc, int ldr);

/* ------------------------------------------------------------------------------------------
 * Input gradient with a fused residual add: dX = dZ x W + dX_out, the gradient that reaches a residual block's input -- the skip
 * connection carries dX_out straight through.  Operands are bgemm_mi355x_nn's (a = dZ [M][lda], b = W [K][ldb] row-major; for the gated
 * layer a = [dG|dU] and b = [Wg;Wu] with K = 2N of that layer); `r` = dX_out is a bf16 matrix [M][ldr], read-only.  There is no bias: a
 * gradient has none.
 * Replaces bgemm_mi355x_nn followed by an element-wise add: a second launch, 6 M N more bytes and a second bf16 rounding.
 * Semantics, exactly:  C[m][n] = bf16_rne( fl32( S[m][n] + float(r[m][n]) ) )
 *   - S is the finished fp32 sum: the accumulator of a plain launch, or the slabs of a two-pass plan added in split order.  ONE fp32 add on
 *     the finished sum, then one rounding.  Nothing is added to a slab.
 * In place, r's rules, the refusals and what is out of scope are bgemm_mi355x_tn_bias_add's: r == c needs ldr == ldc, each C[m][n] is
 * computed from the old r[m][n]; r is 16-byte aligned with ldr % 8 == 0 and (BM ldr + N) 2 bytes below 2 GiB, or the reference kernel answers.
 * The table, ids, names, plan, workspace size and reserve call are hgemm_mi355x_nn_*'s: the tiles, cuts and slabs of a call are those of the
 * bgemm_mi355x_launch_nn call with the same arguments, and so are the splits word, HGEMM_PLAN_NT_STORE, the statuses and the capture
 * behaviour. */
/* planned, contiguous (lda = K, ldb = ldc = ldr = N) */
int bgemm_mi355x_nn_add(const void* a, const void* b, const void* r, void* c, int M, int N, int K, void* stream);
int bgemm_mi355x_launch_nn_add(int nn_config, int splits, const void* a, const void* b, const void* r, void* c, int M, int N, int K,
                               int lda, int ldb, int ldc, int ldr, void* stream);
/* bgemm_mi355x_nn_dact_runs(nn_config, M, N, K, lda, ldb, ldc, ldr): r has z's conditions; 0 for ldr < N */
int bgemm_mi355x_nn_add_runs(int nn_config, int M, int N, int K, int lda, int ldb, int ldc, int ldr);

const char* hgemm_mi355x_strerror(int status);
int hgemm_mi355x_last_hip_error(void);   /* hipError_t behind the calling thread's last HGEMM_ERR_HIP */
const char* hgemm_mi355x_version(void);

/* ------------------------------------------------------------------------------------------
 * Vendor baselines (same tensors, same process, as in the reference's cublas/ tree).
 *
 * rocBLAS  <-  cublasGemmEx NN / TN (reference cublas/fp32/hgemm_cublas.cu:15-68):
 * row-major C = A.B computed as the column-major product C^T = B^T.A^T. */
int hgemm_rocblas_init(void);      /* init_cublas_handle    (hgemm_cublas.cu:15-28) */
int hgemm_rocblas_destroy(void);   /* destroy_cublas_handle (hgemm_cublas.cu:30-38) */
int hgemm_rocblas_nn(const void* a, const void* b, void* c, int M, int N, int K, int acc, void* stream);
int hgemm_rocblas_tn(const void* a, const void* b_col_major, void* c, int M, int N, int K, int acc, void* stream);
/* the TA layout (a_col_major [K][M], b row-major): the same rocblas_gemm_ex with its second operand transposed, ld = M */
int hgemm_rocblas_ta(const void* a_col_major, const void* b, void* c, int M, int N, int K, int acc, void* stream);
/* the vendor counterparts of bgemm_mi355x_nn / _ta: the same rocblas_gemm_ex calls with bf16 operands and C, fp32 compute */
int bgemm_rocblas_nn(const void* a, const void* b, void* c, int M, int N, int K, void* stream);
int bgemm_rocblas_ta(const void* a_col_major, const void* b, void* c, int M, int N, int K, void* stream);
/* ... and of bgemm_mi355x_tn: hgemm_rocblas_tn's call with bf16 operands and C */
int bgemm_rocblas_tn(const void* a, const void* b_col_major, void* c, int M, int N, int K, void* stream);

/* hipBLASLt heuristic  <-  cublasLtMatmulAlgoGetHeuristic top-1 of 4, cached
 * (reference cublas/fp32/hgemm_cublaslt_heuristic.cu:65-217). */
int hgemm_hipblaslt_heuristic_init(void);     /* init_cublaslt_handle_v1    */
int hgemm_hipblaslt_heuristic_destroy(void);  /* destroy_cublaslt_handle_v1 */
int hgemm_hipblaslt_heuristic_nn(const void* a, const void* b, void* c, int M, int N, int K, int acc, void* stream);
int hgemm_hipblaslt_heuristic_tn(const void* a, const void* b_col_major, void* c, int M, int N, int K, int acc, void* stream);

/* hipBLASLt autotune  <-  find_best_algo_{nn,tn}_v2 + cublaslt_tensor_op_{nn,tn}_v2
 * (reference cublas/fp32/hgemm_cublaslt_auto_tuning.cu:108-546): every candidate algorithm is
 * timed for 50 warm-up + 100 measured rounds, shuffled order, fresh N(0,1) inputs each round,
 * median per algorithm, best kept. */
int hgemm_hipblaslt_autotune_init(void);      /* init_cublaslt_handle_v2    */
int hgemm_hipblaslt_autotune_destroy(void);   /* destroy_cublaslt_handle_v2 */
int hgemm_hipblaslt_autotune_find_best_nn(int M, int N, int K, int acc);
int hgemm_hipblaslt_autotune_find_best_tn(int M, int N, int K, int acc);
int hgemm_hipblaslt_autotune_nn(const void* a, const void* b, void* c, int M, int N, int K, int acc, void* stream);
int hgemm_hipblaslt_autotune_tn(const void* a, const void* b_col_major, void* c, int M, int N, int K, int acc, void* stream);
/* On-disk cache of the search results (round 6).  The reference repeats the search in every benchmarking process
 * (benchmarking_offline.py:71-84: find_best_algo_* right after the handles are created), 7 + 1 processes per shape; over a
 * 1000-shape grid x two accumulate trees x two modes that is the same search eight thousand times.  With a cache file -- the
 * environment's HGEMM_AUTOTUNE_CACHE, or hgemm_hipblaslt_autotune_set_cache(path) (NULL / "" = none) -- find_best_* first looks the
 * problem (layout, M, N, K, compute type) up: a record searched with at least the current HGEMM_AUTOTUNE_MAX_SECONDS whose
 * hipBLASLt solution index resolves to the recorded solution name in the running library (an index is only valid for the build of
 * hipBLASLt that searched it: the torch wheel bundles its own, bin/hgemm_tune links /opt/rocm's -- records of both may share a
 * file) and which the library accepts for the problem is taken as the winner without timing anything;
 * otherwise the search runs and appends its winner (text, one line per problem: tn M N K compute16 algo_index best_ms candidates
 * warm timed budget_s solution_name).  hgemm_hipblaslt_autotune_from_cache(tn): 1 when the last find_best of that layout was a
 * cache hit; _cache_stats: records held, hits / misses of this process. */
int hgemm_hipblaslt_autotune_set_cache(const char* path);
int hgemm_hipblaslt_autotune_from_cache(int tn);
int hgemm_hipblaslt_autotune_cache_stats(int* hits, int* misses);
/* Introspection for reports: candidates tried / median ms of the winner (nn = 0, tn = 1). */
int hgemm_hipblaslt_autotune_candidates(int tn);
double hgemm_hipblaslt_autotune_best_ms(int tn);
/* 1 when the last hipBLASLt problem prepared with acc = HGEMM_ACC_FP16 for this layout found no
 * HIPBLAS_COMPUTE_16F kernel and runs with 32F compute instead (result files report it as
 * "hipblaslt_compute16_fallback"), 0 when 16F compute is in use or acc was FP32, -1 before any call.
 * which: 0 = heuristic, 1 = autotune; tn: 0 = nn, 1 = tn. */
int hgemm_hipblaslt_compute16_fallback(int which, int tn);

/* Device helper used by the autotune baseline and the native tools: fill `n` fp16 values with
 * N(0,1) samples (counter-based generator; `seed` makes runs reproducible). */
int hgemm_fill_normal_f16(void* device_ptr, size_t n, unsigned long long seed, void* stream);

/* ---- measurement helpers (bench.py; the reference times with torch events around each call,
 * benchmarking_utils.py:23-31) ------------------------------------------------------------------
 * hgemm_mi355x_time_next_launch arms a one-shot hook: the next GEMM call of the calling thread puts
 * the two events on its main kernel's own dispatch packet, so hgemm_mi355x_event_elapsed_us returns
 * that plan's device time as rocprofv3 reports it (event-record marker packets around a launch
 * add ~6 us of queue gaps on MI355X).  Plans with several kernels (two-pass split-K, hybrid tail) carry the
 * start event on their first dispatch and the stop event on their last one, so the combine is included.
 * Pass (NULL, NULL) to disarm.  Events are created / destroyed with the two helpers below. */
void* hgemm_mi355x_event_create(void);
int hgemm_mi355x_event_destroy(void* event);
int hgemm_mi355x_time_next_launch(void* start_event, void* stop_event);
/* Waits for stop_event, returns microseconds between the two events (negative on error). */
double hgemm_mi355x_event_elapsed_us(void* start_event, void* stop_event);

/* ---- the one-tile-per-workgroup kernel of q256x256_w2x2 ---------------------------------------------------------------------
 * A launch of geometry q256x256_w2x2 in which every workgroup computes at most one output tile (4096^3: 256 tiles on 256
 * workgroups) runs a kernel of its own, without the persistent item walk and without LDS-DMA behind the last K-step.  It is taken
 * when ALL of these hold: plain fp16 epilogue (no split-K, no hybrid tail pass, no stream-K) in its wide form (N % 8 == 0,
 * ldc % 8 == 0, C 16-byte aligned); K % 64 == 0 and K >= 192 (three K-steps: the depth of the kernel's operand streams); work items
 * <= launched workgroups (at most 256 tiles); none of HGEMM_PLAN_RS_XCD_STAGGER, HGEMM_PLAN_PHASE_OFFSET, HGEMM_PLAN_PHASE_OFFSET4.
 * Every other launch runs the general kernel.  C is bit-identical either way; plan, config id, flags, workspace are unchanged.
 *
 * hgemm_mi355x_set_one_item_kernel(on) is a process-wide switch (default on; off in a -DHGEMM_TIMELINE measurement build) and
 * returns the previous value, so tests and A/B timing run both kernels from one library.
 * hgemm_mi355x_one_item_kernel_launches() counts the launches of the kernel since the library was loaded.
 * hgemm_mi355x_one_item_kernel_takes() answers, without a GPU, whether hgemm_mi355x_launch with these arguments (b_col_major given,
 * all pointers 16-byte aligned) would run it under the current switch: 1 / 0, negative status for arguments the launch rejects. */
int hgemm_mi355x_set_one_item_kernel(int on);
unsigned long long hgemm_mi355x_one_item_kernel_launches(void);
int hgemm_mi355x_one_item_kernel_takes(int config_id, int splits, int group_m, int M, int N, int K, int lda, int ldb, int ldc);

#ifdef __cplusplus
}
#endif
#endif /* HGEMM_MI355X_H_ */
