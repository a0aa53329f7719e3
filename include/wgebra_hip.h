/*
 * wgebra_hip.h -- C ABI of libwgebra_hip.so: the MI355X (gfx950) backend behind the wgebra operator
 * surface (Gemm / Gemv / Reduce / OpAssign on wgcore GpuTensor / GpuTensorView).
 *
 * It replaces exactly the slab of the reference that sits under that surface:
 *   wgpu::Buffer storage          (wgcore tensor.rs:117-122,150-154)      -> wg_buf_*      (hipMalloc / hipHostMalloc)
 *   CommandEncoder/ComputePass +
 *   Queue::submit + Device::poll  (wgcore kernel.rs:15-27,125-146;
 *                                  tensor.rs:300-325)                      -> wg_ctx_*      (one in-order hipStream_t)
 *   ViewShape uniform buffers     (wgcore shapes.rs:9-21,107-116)          -> wg_view_shape passed BY VALUE as kernel args
 *   the 10 WGSL entry points      (wgebra linalg/{gemm,gemv,reduce,
 *                                  op_assign}.wgsl)                        -> wg_gemm / wg_gemv / wg_reduce / wg_op_assign
 *   GpuTimestamps                 (wgcore timestamps.rs:9-248)             -> wg_timestamps_* (hipEvent pairs)
 *
 * Conventions
 *   - Plain C: opaque handles, plain pointers and sizes, `int` status returns (0 == WG_OK). No C++/torch types.
 *   - All tensors are COLUMN-MAJOR; a view is (buffer, wg_view_shape); element (i,j,t) lives at element index
 *     t*stride_mat + offset + i + j*stride of the buffer (shape.wgsl:45-47,60-62). Units: ELEMENTS of the dtype.
 *   - A context owns one in-order stream: operators enqueue asynchronously w.r.t. the host, in call order,
 *     exactly like dispatches recorded into one ComputePass; wg_ctx_sync / wg_buf_read block.
 *   - A context is not thread-safe; distinct contexts are independent (one per GPU for multi-GPU).
 *   - Errors: where the reference panics (assert_eq!) the call returns a status and records a message with the
 *     reference's text (wg_last_error_string); where the reference silently skips a dispatch (zero-sized buffer
 *     or grid, kernel.rs:111-123,144) the call returns WG_OK and launches nothing.
 *   - Where the reference would read or write out of bounds (its shaders run with bounds checks disabled,
 *     wgcore utils.rs:11-19) the call returns WG_ERR_OUT_OF_BOUNDS / WG_ERR_PRECONDITION instead.
 *   - OVERLAPPING OPERANDS ("the aliasing rule"; every operator's comment below refers to it). The footprint of a view is the set of elements
 *     t*stride_mat + offset + i + j*stride it addresses -- for Reduce, OpAssign, Axpy and Gemv the elements the call really addresses (offset + i for a vector;
 *     Gemv takes the column and matrix counts of `m` and `v` from `out`), the views the bounds checks use. A call whose WRITTEN footprint shares a byte with a
 *     footprint it READS returns WG_ERR_ALIASED: nothing is launched, nothing is logged (wg_debug_take_path), no memory changes, a recording stays open and
 *     usable; the message names the operator and both views ("Gemm: `out` overlaps `m1`"). The reference cannot get that far -- its kernels bind the output
 *     read_write and the inputs read (gemm.wgsl:10-14, gemv.wgsl:10-14, op_assign.wgsl:8-10, reduce.wgsl:6-8), and wgpu refuses a dispatch that binds one
 *     buffer both ways. Overlap is decided on ADDRESSES (device pointer + byte range), never on wg_buf identity: two handles over one allocation (wg_buf_wrap)
 *     overlap like two views of one handle. Extension over wgpu, which tracks whole buffers: views of ONE buffer whose footprints are disjoint are legal --
 *     views that touch, and views that interleave (an output that lives in the leading-dimension padding of an input).
 *     The one exception (extension): wg_op_assign and wg_axpy take the IDENTICAL view -- same address, same length -- as `a` and `b` (`y` and `x`):
 *     every element is loaded (both operands) before it is stored, by the lane that stores it, so `a += a`, `a *= a`, `y += alpha y` are well defined and
 *     bit-equal to x (op) x. A partial overlap of `a` and `b` is refused.
 *     Cost and the conservative bound: disjoint byte intervals are accepted after a few integer comparisons. Views whose intervals intersect are compared
 *     exactly, column run by column run, while the two views have at most WG_VIEWS_OVERLAP_MAX_RUNS runs between them (a dense matrix or cube counts as one
 *     run); beyond that the call is refused although the footprints might interleave without touching (the message then says "may overlap").
 */
#ifndef WGEBRA_HIP_H
#define WGEBRA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WGEBRA_HIP_ABI_VERSION 5 /* 5: wg_debug_take_path; and the round-6 additions that came without a bump: wg_copy_view, wg_timestamps_reserve,
                                    wg_timestamps_write_at, WG_TUNE_RM_TR_NATIVE, wg_debug_gemm16_plan and wg_debug_gemm32_plan (added diagnostic symbols with their two structs each); WG_ERR_ALIASED = 9 (an appended status: calls that
                                    return it used to launch kernels that raced on their own operands) with wg_debug_views_overlap; and WG_BF16 = 2 in wg_dtype (a new enum value: backward compatible -- every call
                                    that was valid keeps its meaning, dtype 2 used to be WG_ERR_INVALID_ARG -- so no bump); wg_gemv_mixed (an added symbol); wg_gemm_out32 with wg_debug_gemm_out32_query (added symbols);
                                    wg_gemv_q8 with wg_debug_gemv_q8_plan and its two structs (added symbols; wg_dtype is unchanged);
                                    wg_gemm_q8 with wg_debug_gemm_q8_plan and its two structs (added symbols; wg_dtype is unchanged);
                                    wg_gemv_q4 with wg_debug_gemv_q4_plan and its two structs (added symbols; wg_dtype is unchanged);
                                    wg_gemm_q4 with wg_debug_gemm_q4_plan and its two structs (added symbols; wg_dtype is unchanged);
                                    wg_gemm_q8a8 with wg_debug_gemm_q8a8_plan, wg_quantize_q8 with wg_debug_quantize_q8_plan, and their two structs each (added symbols; wg_dtype is unchanged);
                                    wg_debug_gemv_plan and wg_debug_gemv_any_plan with wg_gemv_query and their plan structs (added diagnostic symbols);
                                    4: wg_gemm_sharded_panels (ragged N-panels), wg_ctx_mem_info, geometry ops 15-18; 3: the SDMA rect-copy exchange engine (gather mode 1, wg_comm_copy_engine, wg_gemm_sharded's peer_out) is gone;
                                    wg_comm_reported_size, wg_debug_*; non-vec4 views compute staged; async time-outs surface in wg_ctx_sync */

/* ------------------------------------------------------------------------------------------------ */
/* status codes                                                                                      */
/* ------------------------------------------------------------------------------------------------ */
typedef enum wg_status {
    WG_OK = 0,
    WG_ERR_DIM_MISMATCH = 1,  /* reference: assert_eq!(.., "Gemm: dimension mismatch.") & friends -> panic   */
    WG_ERR_PRECONDITION = 2,  /* an assertion of the reference that is not a dimension check: GemvFast rows % 4 (gemv.rs:122), ... */
    WG_ERR_INVALID_ARG = 3,   /* null handle, unknown enum value, foreign-context buffer                      */
    WG_ERR_OUT_OF_BOUNDS = 4, /* the view addresses elements past the end of its buffer                       */
    WG_ERR_HIP = 5,           /* a HIP runtime call failed; message carries hipGetErrorString                 */
    WG_ERR_UNSUPPORTED = 6,   /* dtype/variant combination not implemented                                    */
    WG_ERR_NO_DEVICE = 7,     /* no gfx950 device visible (GpuInstance::new() -> Err, gpu.rs:24-58)           */
    WG_ERR_WORKSPACE = 8,     /* a context scratch region would have to grow while recording (allocation cannot be
                                 captured): run the call once eagerly, or wg_ctx_reserve_workspace, then record    */
    WG_ERR_ALIASED = 9        /* the written view shares memory with a view the call reads (the aliasing rule above; the reference:
                                 a wgpu validation panic). Nothing was launched                                     */
} wg_status;

/* ------------------------------------------------------------------------------------------------ */
/* enums: same names and ORDER as the Rust enums                                                     */
/* ------------------------------------------------------------------------------------------------ */
/* reference kernels are f32 only; F16 and BF16 are this build's extensions. WG_BF16 (bfloat16: 8 exponent bits, 8 significant bits) is accepted by every entry
 * point that takes WG_F16, for the same views, shapes, variants, alpha / beta and tuning values, with the same status codes and messages. Its contract:
 *   - bf16 -> f32 is exact (the 16 bits become the high half of the f32); f32 -> bf16 is ONE round-to-nearest-even at the store: NaN stays a quiet NaN,
 *     +-Inf stays +-Inf, a finite f32 past the largest bf16 (~3.39e38) becomes Inf, subnormals are flushed neither when read nor when written;
 *   - Gemm / Gemv: products of bf16 operands are exact in f32, accumulation is f32 in the same orders as the f16 kernels (v_mfma_f32_16x16x32_bf16), the epilogue
 *     forms alpha*acc + beta*c in f32 and rounds once; beta == 0 never reads `out`; (1, 0) is bit-identical to wg_gemm;
 *   - Reduce family: elements are widened, folded in f32 in the reference order (the fixed chunked order for wg_reduce_fast), the result is rounded once;
 *     an empty vector gives the op's initial value rounded to bf16;
 *   - OpAssign / Axpy: computed in f32 on the widened elements, rounded once;
 *   - wg_copy_view / wg_cube_to_matrix / wg_all_gather (ncclBfloat16) move the 16 bits unchanged;
 *   - wg_gemm_sharded / wg_gemm_sharded_panels take it panel by panel (the one-launch forms are f16 only; bf16 silently takes the panel launches, as f32 does);
 *   - wg_debug_take_path: the f16 tags with the element prefix "f16." replaced by "bf16." ("bf16.cont", "bf16.pad/c=seed>bf16.t128/ns=1"); the dtype-free tags
 *     ("gemv.n/...", "reduce.rows4/...", "splitk.reduce/...") are the same for every element type.
 * WG_F32 and WG_F16 likewise: subnormal operands and results are flushed neither when read nor when written, on every operator -- Gemm and Gemv on the matrix
 * cores included (measured on gfx950: f16 and bf16 subnormal A / B inputs of the MFMAs take part with their exact values), Reduce (Min / Max return a subnormal
 * extreme as it is), OpAssign (gradual underflow, correctly rounded subnormal quotients) and Axpy; a result below the smallest normal is rounded ONCE onto the
 * subnormal grid, ties to even (tests/test_gpu_exponent_range.py). */
typedef enum wg_dtype { WG_F32 = 0, WG_F16 = 1, WG_BF16 = 2 } wg_dtype;

typedef enum wg_gemm_variant { /* wgebra gemm.rs:26-35 */
    WG_GEMM = 0, WG_GEMM_FAST = 1, WG_GEMM_TR = 2, WG_GEMM_TR_FAST = 3
} wg_gemm_variant;

typedef enum wg_gemv_variant { /* wgebra gemv.rs:25-34 */
    WG_GEMV = 0, WG_GEMV_FAST = 1, WG_GEMV_TR = 2, WG_GEMV_TR_FAST = 3
} wg_gemv_variant;

typedef enum wg_reduce_op { /* wgebra reduce.rs:13-27 */
    WG_REDUCE_MIN = 0, WG_REDUCE_MAX = 1, WG_REDUCE_SUM = 2, WG_REDUCE_PROD = 3, WG_REDUCE_SQNORM = 4
} wg_reduce_op;

typedef enum wg_op_assign_variant { /* wgebra op_assign.rs:12-26 */
    WG_OP_ADD = 0, WG_OP_SUB = 1, WG_OP_MUL = 2, WG_OP_DIV = 3, WG_OP_COPY = 4
} wg_op_assign_variant;

/* wgpu::BufferUsages bit values (the flags TensorBuilder takes, tensor.rs:65-112). Only MAP_READ / MAP_WRITE
 * change behaviour here: a MAP_* buffer is pinned host memory (the "staging" tensor of gemm.rs:163-168). */
enum {
    WG_USAGE_MAP_READ = 1u << 0, WG_USAGE_MAP_WRITE = 1u << 1, WG_USAGE_COPY_SRC = 1u << 2,
    WG_USAGE_COPY_DST = 1u << 3, WG_USAGE_INDEX = 1u << 4, WG_USAGE_VERTEX = 1u << 5,
    WG_USAGE_UNIFORM = 1u << 6, WG_USAGE_STORAGE = 1u << 7, WG_USAGE_INDIRECT = 1u << 8,
    WG_USAGE_QUERY_RESOLVE = 1u << 9
};

/* ------------------------------------------------------------------------------------------------ */
/* wg_view_shape: byte-identical to wgcore::shapes::ViewShape (#[repr(C)], 24 B; shapes.rs:9-21)    */
/*                and to WGSL `Shape` (shape.wgsl:10-33).                                            */
/* ------------------------------------------------------------------------------------------------ */
typedef struct wg_view_shape {
    uint32_t size[3];    /* rows, cols, mats */
    uint32_t stride;     /* elements between two columns */
    uint32_t stride_mat; /* elements between two matrices */
    uint32_t offset;     /* index of the first element of the view in the buffer */
} wg_view_shape;

typedef struct wg_ctx wg_ctx;               /* GpuInstance (gpu.rs:7-12) + the encoder/pass/queue it feeds */
typedef struct wg_buf wg_buf;               /* wgpu::Buffer */
typedef struct wg_cmdbuf wg_cmdbuf;         /* wgpu::CommandBuffer (a recorded, replayable hipGraphExec) */
typedef struct wg_timestamps wg_timestamps; /* wgcore::timestamps::GpuTimestamps */

/* ------------------------------------------------------------------------------------------------ */
/* library / device                                                                                  */
/* ------------------------------------------------------------------------------------------------ */
int wg_abi_version(void);
/* Thread-local message of the last failing call on this thread ("" if none). Never NULL. */
const char *wg_last_error_string(void);
/* Number of visible HIP devices (0 without a GPU; never fails). */
int wg_device_count(void);

/* GpuInstance::new() (gpu.rs:24-58): bind `device`, create the in-order stream. */
int wg_ctx_create(int device, wg_ctx **out);
/* Same, but enqueue on an existing hipStream_t (e.g. the stream another runtime owns). Not destroyed with the ctx. */
int wg_ctx_create_on_stream(int device, void *hip_stream, wg_ctx **out);
/* A context whose stream may use only `cu_count` of the device's compute units (CU-masked stream; every XCD loses the same
 * share). For multi-GPU runs: the compute stream leaves a few CUs to the collective library's copy kernels. The tile / split
 * heuristics then plan for `cu_count` CUs. */
int wg_ctx_create_with_cu_count(int device, uint32_t cu_count, wg_ctx **out);
/* Same, but the missing CUs (fewer than one XCD's worth) all come from ONE XCD: the other seven keep their 32 CUs and the L2 locality of
 * the f16 Gemm's tile patches, and that kernel's tile scheduler lets them take the short XCD's tiles (248 CUs: 13.8 -> 13.5 ms per step of a
 * rank's 8192 x 32768 x 32768 product). For a context that runs the sharded f16 Gemm beside a collective; kernels with a static
 * tile -> XCD map run better on the evenly masked stream above. */
int wg_ctx_create_with_cu_count_one_xcd(int device, uint32_t cu_count, wg_ctx **out);
int wg_ctx_destroy(wg_ctx *ctx);
/* queue.submit(..) + device.poll(PollType::wait()) (tensor.rs:304-312): block until all enqueued work is done. Also reports (once) an
 * error a kernel of this context raised asynchronously -- a sharded Gemm whose peer never delivered (WG_ERR_HIP); so does wg_buf_read. */
int wg_ctx_sync(wg_ctx *ctx);
int wg_ctx_device(const wg_ctx *ctx);
void *wg_ctx_stream(const wg_ctx *ctx); /* the hipStream_t, for interop */
/* Device facts the bench prints next to every roofline: name (<=255 chars), CU count, clock MHz, HBM bytes. */
int wg_ctx_device_info(const wg_ctx *ctx, char *name256, int *compute_units, int *clock_mhz, uint64_t *hbm_bytes);
/* Free and total device memory in bytes right now (hipMemGetInfo on the context's device): what `wgpu::Device::limits` cannot say; the sharded
   GEMM sizes its panels from it and the tests check that dropped buffers really come back. */
int wg_ctx_mem_info(const wg_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes);
/*
 * Geometry: the reference's `wgebra::geometry` WGSL modules (the .wgsl files under crates/wgebra/src/geometry) are device
 * functions used inside other shaders; their HIP counterpart is the header include/wgebra_geometry.hpp (`__host__ __device__`).
 * This entry point applies one of them to `count` independent items, one per thread -- the same harness the reference's tests
 * use (a one-invocation-per-matrix test kernel). Item layouts: wgmath_amd/csrc/geometry.hip.
 */
typedef enum wg_geom_op {
    WG_GEOM_INV = 0, WG_GEOM_CHOLESKY = 1, WG_GEOM_LU = 2, WG_GEOM_QR = 3, WG_GEOM_SYM_EIGEN = 4, WG_GEOM_SVD = 5,
    WG_GEOM_ROT2 = 6, WG_GEOM_QUAT = 7, WG_GEOM_SIM2 = 8, WG_GEOM_SIM3 = 9,
    /* the transform functions one by one on raw coordinates (a non-unit quaternion, a (cos, sin) pair that is no rotation): the items the
       fixtures executed from the reference's WGSL text hold (tests/golden/wgsl_exec_geometry.npz); FROM = quat::fromScaledAxis + rot2::fromAngle */
    WG_GEOM_QUAT_RAW = 10, WG_GEOM_ROT2_RAW = 11, WG_GEOM_SIM2_RAW = 12, WG_GEOM_SIM3_RAW = 13, WG_GEOM_FROM = 14,
    /* UTILS = wgebra::trig (utils/trig.wgsl:12-38: stable_atan2, stable_tanh) + wgebra::min_max (utils/min_max.wgsl:4-51); ROT2_EXT = rot2.wgsl's
       angle / cancel_y / is_valid / rotate_rows3 / rotate_rows4 (:15-36, :51-53, :78-95); EIGVALS2 = eig2.wgsl:44-56 `eigenvalues`;
       SVD_RECOMPOSE (dim 2, 3) = svd2.wgsl:43-46 / svd3.wgsl:309-312 `recompose` on items in the layout WG_GEOM_SVD writes */
    WG_GEOM_UTILS = 15, WG_GEOM_ROT2_EXT = 16, WG_GEOM_EIGVALS2 = 17, WG_GEOM_SVD_RECOMPOSE = 18
} wg_geom_op;
int wg_geometry_apply(wg_ctx *ctx, wg_geom_op op, uint32_t dim, const wg_buf *in, wg_buf *out, uint32_t count);

/*
 * Diagnostics only (tools/overlap_probe.py): enqueue `blocks` workgroups of 256 threads that spin for `usec` microseconds and
 * record their start tick (s_memrealtime, 100 MHz) into start_ticks[0 .. blocks) (u64 each; start_ticks[blocks] = tick of a
 * 1-thread kernel enqueued just before). Stand-in for a collective library's copy kernel when studying queue interleaving.
 */
int wg_debug_spin(wg_ctx *ctx, uint32_t blocks, uint32_t usec, wg_buf *start_ticks);
/* What the chip did while a kernel ran (the role of GpuTimestamps, timestamps.rs:226-230, for a power-capped part: a time alone does not say
 * whether a slow run was a slow kernel or a slow clock).
 * wg_debug_clock_begin / _end bracket whatever is enqueued between them on the context's stream with two stamp kernels (s_memtime -- shader
 * clock ticks -- against s_memrealtime -- 100 MHz --, per XCD): _end synchronises the stream and returns the MEAN shader clock over the
 * bracketed interval in GHz (mean / min / max over the XCDs; any of the last three pointers may be NULL) and the interval's length. Nothing
 * is added to the bracketed kernels and nothing runs beside them.
 * wg_debug_mfma_ceiling runs v_mfma_f32_16x16x32_f16 alone (random operands in registers, no LDS or memory traffic, one 4-wave workgroup per
 * CU of the context's stream) for at least min_seconds (0 < s <= 30) and returns its TFLOP/s and mean shader clock: what the package power cap
 * leaves the matrix cores when nothing else draws power -- the ceiling of any f16 Gemm on this part. */
int wg_debug_clock_begin(wg_ctx *ctx);
int wg_debug_clock_end(wg_ctx *ctx, double *ghz_mean, double *ghz_min, double *ghz_max, double *seconds);
int wg_debug_mfma_ceiling(wg_ctx *ctx, double min_seconds, double *tflops, double *clock_ghz);
/* Which leaves of the Gemm / Gemv / Reduce launchers' dispatch trees ran since the last call (tests): one short tag per terminal launch, space-separated --
 * "f32.big/ns=4 splitk.reduce/ns=4", "f16.cont", "f16.pad/c=seed>f16.t128/ns=1" (a tag ending in '>' wraps the next one: staging, padding, transposed
 * forms). Gemv names its kernel instance: "gemv> f32.gemv gemv.n/t=4,ns=3 gemv.combine/ns=3", "gemv.small/rl=8", "gemv.t/t=8,ns=1",
 * "gemv.tcols/e=8,u=4,v=2,ns=1" (elements per load, loads in flight, right-hand sides), "gemv.tlds/nr=4,c=2,th=1024", "gemv.small_reduce/rl=4",
 * "gemv> f16w.gemv gemv.tcols/e=8,u=8,v=1,ns=1" (wg_gemv_mixed: 16-bit weights, f32 vectors), "gemv_reduce.two>" (wg_gemv_reduce as Gemv, then Reduce), "gemv_any/t,ns=2" (views the vec4 kernels cannot take); Reduce: "reduce.long",
 * "reduce.rows4/al=1" (al: the aligned vec4 instance), "reduce.fast/np=64". Equal logs mean the same kernels in the same summation order. Host-side bookkeeping only; the context keeps the newest few hundred bytes.
 * Copies the log into buf (NUL-terminated, truncated to cap - 1 bytes) and clears it; buf may be NULL to just clear it. */
int wg_debug_take_path(wg_ctx *ctx, char *buf, size_t cap);

/*
 * Kernel-selection knobs of a context (tests and experiments; production code never needs them). The launchers choose between
 * kernel families by shape; a knob forces one choice for every later call on this context. Defaults come from the environment
 * ONCE, when the context is created (WG_F16_TILE, WG_F16_SCHED, WG_F32_SKINNY, WG_F32_PANELS, WG_F16_BALANCE): the dispatch path itself never
 * reads the environment.
 * The WG_TUNE_F16_* knobs mean "the 16-bit Gemm family": the bf16 kernels are the f16 sources compiled for the other element type, share the launcher's dispatch
 * tree and are steered by the same knobs in the same way.
 */
typedef enum wg_tuning {
    WG_TUNE_F16_TILE = 0,    /* 0 = by shape (default), 128 / 256 = force the 128 x 128 / 256 x 256 f16 kernel family, 256128 = the 256 x 128 tile (two
                                workgroups per CU: short K) whenever its kernel takes the shape */
    WG_TUNE_F16_SCHED = 1,   /* -1 = by size (default), 0 / 1 = static tile map / tile queues with stealing across XCDs */
    WG_TUNE_F32_SKINNY = 2,  /* -1 = by shape, 0 / 1 = never / whenever applicable: the few-column f32 kernel */
    WG_TUNE_F32_PANELS = 3,  /* -1 = by estimate, 0 / 1: 64-column panels of the few-column kernel for small square f32 products */
    WG_TUNE_F16_BALANCE = 4, /* calibrated per-XCD shares (K-prefix units) for f16 products of few rounds: 0 = off (default: measured not to pay on
                                MI355X, gemm_f16.hip), -1 = measure slot rates and let the planner decide, 1 = the tests' fixed pattern */
    WG_TUNE_F32_MID = 5,     /* the mid-size f32 tile family (gemm_f32_mid.hip: 128 x 128, 128 x 64, 64 x 128 tiles on 2 x 2 waves; 96 x 96, 96 x 64, 64 x 96, 64 x 64, 64 x 32,
                                32 x 64 with K split over the workgroup's waves; the whole K in one workgroup unless WG_TUNE_F32_MID_SPLIT / its estimate cuts K across workgroups
                                (few tiles, long K: slabs + a reduce launch); for outputs of <= 64 rows or columns it is tried BEFORE the few-column kernels unless
                                WG_TUNE_F32_SKINNY or _PANELS is forced to 1): -1 = by estimate (default), 0 = never, 1 = whenever
                                applicable with the estimate's tile, 128128 / 128064 / 64128 / 96096 / 96064 / 64096 / 64064 / 64032 / 32064 = that tile (tests) */
    WG_TUNE_F32_MID_SPLIT = 6, /* K cut of the mid family's k-split tiles across workgroups (few tiles, long K: 64 x 4096 x 4096): 0 = by estimate (default), n >= 2 = n
                                 splits whenever that family runs (tests) */
    WG_TUNE_GEMVT_LDS = 7,   /* GemvTr with 2 .. 8 right-hand sides on the vectors-in-LDS kernel (gemv.hip gemv_t_lds_kernel): 0 = where it measured ahead (default: from
                                128 outputs per CU on; two right-hand sides from 8), n >= 1 = from n outputs per CU on whatever the count of right-hand sides,
                                vectors longer than the LDS in up to 4 chunks (tests: every workgroup shape of the kernel) */
    WG_TUNE_F16_CONT = 8,    /* f16 Gemm / GemmTr on the continuous tile walk (gemm_f16.hip m16_cont: one workgroup per CU keeps its LDS-DMA stream going across its tiles):
                                -1 = by shape (default: K <= 4096, or <= 8192 below 16 rounds of tiles; more than one round of whole tiles), 0 = never,
                                1 = whenever applicable (tests) */
    WG_TUNE_RM_TR_NATIVE = 9, /* row-major GemmTr (wg_gemm_rm) on the kernels that take the second operand contiguous along N (gemm_f16_nt.hip, the B_NC instances of gemm_f16_t128.hip / gemm_f32.hip) instead of
                                transposing m1 into a scratch buffer first: -1 = from about half a round of tiles on (default: f16 128 x 128 tiles, f32 one round of 256 x 128 tiles), 0 = never
                                (the transposed copy: tests compare the two), 1 = whenever those kernels take the shape */
    WG_TUNE_COUNT_ = 10
} wg_tuning;
int wg_ctx_set_tuning(wg_ctx *ctx, wg_tuning key, int value);
/* Diagnostics / tests (no device needed): the f16 Gemm's calibrated-shares plan for `tiles` whole 256 x 256 tiles of `stages` stages (64 k
 * each) from eight relative slot rates (time per stage of the workgroup slots b % 8, mean 1), or the fixed test pattern (forced != 0),
 * decoded for every workgroup exactly as the kernel decodes it: units[5 i ..] = (tile, mode 0 whole / 1 prefix / 2 suffix, first stage,
 * stages, pair) of the i-th workgroup that has work; *nunits = how many there are (may exceed `capacity`), *nworkgroups = the grid. */
/* The per-slot rates the context has measured so far (time per stage of the workgroup slots b % 8 relative to their mean; all 1 until
 * `*valid`), how many snapshots went into them, and how many launches ran with calibrated shares. */
int wg_ctx_f16_balance_info(const wg_ctx *ctx, double *rel8, int *valid, uint32_t *updates, uint32_t *balanced_launches);
int wg_debug_f16_balance_plan(const double *rel8, uint32_t tiles, uint32_t stages, int forced, uint32_t *units, uint32_t capacity, uint32_t *nunits,
                              uint32_t *nworkgroups);
/* Diagnostics / tests (no context, no device): which leaf of the 16-bit Gemm launcher (f16 and bf16 share it) a call would take and with what.
 * The launcher itself is "fill a wg_gemm16_query, ask the planner, do what the wg_gemm16_plan says"; this entry point asks the same planner.
 * Everything a choice depends on is in the query; nothing in it needs a device. */
typedef struct wg_gemm16_query {
    uint32_t trans, M, N, K, nmats;          /* out (M x N) = op(m1) (M x K) * m2 (K x N); trans: m1 stored K x M */
    uint32_t lda, ldb, ldc;                  /* leading dimensions of m1, m2 and out (elements) */
    uint64_t a_batch, b_batch, c_batch;      /* matrix strides (elements) */
    uint32_t a_addr, b_addr, c_addr;         /* the low 4 bits of the three base addresses (bytes) */
    float alpha, beta;
    uint32_t panels;                         /* the one-launch N-panel form (wg_gemm_sharded_panels): the widths follow */
    uint32_t panel_cols, panel_n_main, panel_n_tail, panel_tail_cols[8];
    uint32_t cus;                            /* compute units of the context's stream */
    int32_t tile, sched, cont, balance;      /* WG_TUNE_F16_TILE, _SCHED, _CONT, _BALANCE */
    uint32_t uneven_xcds;                    /* a CU-masked stream whose missing CUs all come from one XCD */
    uint32_t recording;                      /* the call is being recorded into a command buffer */
    uint32_t bal_valid;                      /* the context has measured per-XCD rates (wg_ctx_f16_balance_info) */
    uint32_t padded;                         /* the inner call of a padded call: it must not pad again */
} wg_gemm16_query;
typedef enum wg_gemm16_leaf {
    WG_GEMM16_SKINNY = 0,      /* few-column streaming kernel (GemmTr, N <= 16) */
    WG_GEMM16_T256X128 = 1,    /* 256 x 128 tiles, two workgroups per CU */
    WG_GEMM16_T128 = 2,        /* 128 x 128 tiles (+ split-K slabs and their reduce) */
    WG_GEMM16_M16 = 3,         /* 256 x 256 tiles: per-tile launch (static map, tile queues or calibrated shares) or the continuous walk, + cut-up tail, + split-K */
    WG_GEMM16_PAD = 4,         /* zero-padded copies of what does not qualify, then the same call on those */
    WG_GEMM16_GENERIC = 5,     /* the generic fallback kernel */
    WG_GEMM16_UNSUPPORTED = 6  /* no launch: the call returns `status` (with `message`, if there is one; WG_OK for an empty product) */
} wg_gemm16_leaf;
typedef struct wg_gemm16_plan {
    uint32_t leaf;                           /* wg_gemm16_leaf */
    uint32_t tiles_m, tiles_n;               /* tiles of the leaf's kernel (skinny: row blocks x 1) */
    uint32_t nsplit, k_per_split;            /* K cut (1, K: none); every split but the last covers k_per_split, the last one the rest */
    uint32_t c_stream, a_nt;                 /* result stored past the caches; op(A) read with the non-temporal hint */
    uint64_t workspace_bytes;                /* split-K slabs or tail partials (the context's workspace) / the padded copies (its padding workspace) */
    /* WG_GEMM16_M16: the launch of the whole tiles [0, tiles - tail), then the tail */
    uint32_t cont;                           /* the continuous tile walk (one workgroup per CU) */
    uint32_t queues;                         /* per-tile launch taking its tiles from the per-XCD queues */
    uint32_t nwg;                            /* workgroups of that launch (per matrix and split; calibrated shares: decided from the measured rates) */
    uint32_t bal_eligible, bal_calib, bal_wanted; /* calibrated shares: the shape allows them; this launch feeds the rate measurement; a plan is asked for */
    uint32_t tail, tail_split, tail_kps;     /* tail tiles cut along K: how many (0: none), their splits and k per split */
    /* WG_GEMM16_PAD */
    uint32_t Mp, Kp, a_ok, b_ok, c_ok;       /* padded sizes; which of op(A), B and the output are used as they are */
    uint32_t c_seed;                         /* the padded output starts as a copy of the old one (beta != 0) */
    /* WG_GEMM16_UNSUPPORTED */
    int32_t status;
    char message[128];
} wg_gemm16_plan;
/* plan: the plan of `query`. tags (may be NULL): the launch log such a call leaves (the format of wg_debug_take_path, element prefix "f16" or "bf16"), the
 * slab reduce of a K cut included; for a padded call the pad tag followed by the inner call's tags. inner (may be NULL): the query of that inner call
 * (pad plans only; else a copy of `query`). Calibrated shares are planned from flat rates (the forced pattern, WG_TUNE_F16_BALANCE = 1, ignores them). */
int wg_debug_gemm16_plan(const wg_gemm16_query *query, const char *prefix, wg_gemm16_plan *plan, char *tags, size_t cap, wg_gemm16_query *inner);
/* The override wg_gemm_out32's launcher applies to the query it has filled, in place, before it asks the same planner: the continuous walk off (cont = 0) and
 * the panel form off (panels = 0, widths cleared). Nothing else changes; wg_debug_gemm16_plan on the result, with prefix "f16o32" / "bf16o32", is that call's plan. */
int wg_debug_gemm_out32_query(wg_gemm16_query *query);
/* The same for the f32 Gemm launcher (gemm32_plan.hip): "fill a wg_gemm32_query, ask the planner, do what the wg_gemm32_plan says". The f32 launcher reads no
 * addresses: shapes, leading dimensions, matrix strides, the CU count and the four WG_TUNE_F32_* knobs decide everything. */
typedef struct wg_gemm32_query {
    uint32_t trans, M, N, K, nmats;          /* out (M x N) = op(m1) (M x K) * m2 (K x N); trans: m1 stored K x M */
    uint32_t lda, ldb, ldc;                  /* leading dimensions of m1, m2 and out (elements) */
    uint64_t a_batch, b_batch, c_batch;      /* matrix strides (elements) */
    float alpha, beta;
    uint32_t cus;                            /* compute units of the context's stream */
    int32_t mid, mid_split, skinny, panels;  /* WG_TUNE_F32_MID, _MID_SPLIT, _SKINNY, _PANELS */
} wg_gemm32_query;
typedef enum wg_gemm32_leaf {
    WG_GEMM32_NOTHING = 0,      /* an empty product: no launch, WG_OK */
    WG_GEMM32_UNSUPPORTED = 1,  /* no launch: the call returns `status` with `message` */
    WG_GEMM32_MID = 2,          /* the mid family (gemm_f32_mid.hip): bm x bn tiles, K cut across workgroups for nsplit > 1 */
    WG_GEMM32_SKINNY = 3,       /* the few-column kernel (gemm_f32_skinny.hip), one panel */
    WG_GEMM32_SKINNY_PANELS = 4,/* ... on 64-column panels */
    WG_GEMM32_SKINNY_T = 5,     /* ... computing the transposed product of a few-row one, written straight into the transposed position */
    WG_GEMM32_FEWROW = 6,       /* the few-row form on transposed copies: C^T = m2^T op(m1)^T as a GemmTr (the inner call), then a transpose of the result */
    WG_GEMM32_BIG = 7           /* 256 x 128 tiles (gemm_f32.hip): one launch, split-K slabs, or full rounds + a cut-up tail */
} wg_gemm32_leaf;
typedef struct wg_gemm32_plan {
    uint32_t leaf;                           /* wg_gemm32_leaf */
    uint32_t bm, bn;                         /* WG_GEMM32_MID: the tile */
    uint32_t nsplit, k_per_split;            /* K cut (1, K: none), final: no empty split; every split but the last covers k_per_split */
    uint32_t npanels;                        /* the few-column kernels: 64-column panels (1: none) */
    uint32_t copy_a;                         /* WG_GEMM32_FEWROW: op(m1) is copied transposed (Gemm; GemmTr's m1 is used where it lies) */
    uint32_t tail_r, tail_sp, tail_kps;      /* WG_GEMM32_BIG: tail tiles cut along K (0: none), their splits (final) and k per split */
    uint32_t flat_tiles;                     /* ... the tail split of a batch: tiles per matrix, the launches number the tiles through the batch (0: grid.y carries the matrix) */
    uint64_t workspace_bytes;                /* split-K slabs or tail partials (the context's workspace) */
    uint64_t pad_workspace_bytes;            /* WG_GEMM32_FEWROW: the transposed copy of op(m1) and the transposed result (the context's padding workspace) */
    int32_t status;                          /* WG_GEMM32_NOTHING / _UNSUPPORTED */
    char message[128];
} wg_gemm32_plan;
/* plan: the plan of `query`. tags (may be NULL): the launch log such a call leaves (the format of wg_debug_take_path), the slab reduce of a K cut included; for a
 * few-row plan the tag string goes on with the transposes and the inner call's tags. inner (may be NULL): the query of that inner call (few-row plans only; else a
 * copy of `query`). */
int wg_debug_gemm32_plan(const wg_gemm32_query *query, wg_gemm32_plan *plan, char *tags, size_t cap, wg_gemm32_query *inner);
/* The same for wg_gemv_q8's launcher (gemv_q8_plan.hip): kernel, right-hand-side tile, cut of the contraction, grid and workspace bytes as a pure function of
 * the query. Sizes and strides count each operand's own elements (1 byte for `m`, 4 bytes for the others); *_addr16: the byte address of the view's first
 * element modulo 16. */
typedef struct wg_gemv_q8_query {
    uint32_t trans;                          /* 0: out = W v (Gemv, GemvFast); 1: out = W^T v (GemvTr, GemvTrFast) */
    uint32_t rows, cols, nrhs, mats;         /* the matrix as stored (rows x cols); right-hand sides and matrices (taken from `out`) */
    uint32_t group_rows;                     /* as passed: a positive multiple of 16, or any value >= rows */
    uint32_t ldm, lds, ldv, ldo;             /* leading dimensions of m, scales, v and out */
    uint64_t m_batch, s_batch, v_batch, o_batch; /* matrix strides */
    uint32_t m_addr16, v_addr16, o_addr16;   /* byte address of the first element of m, v and out, modulo 16 (scales are read 4 bytes at a time: any view) */
    uint32_t cus;                            /* compute units of the context's stream */
} wg_gemv_q8_query;
typedef enum wg_gemv_q8_leaf {
    WG_GEMV_Q8_NOTHING = 0,      /* no output element: no launch, WG_OK */
    WG_GEMV_Q8_UNSUPPORTED = 1,  /* no launch: the call returns `status` with `message` */
    WG_GEMV_Q8_T = 2,            /* out = W^T v, a half-wave per column or per 4 adjacent columns, 16-byte loads (gemv_q8_t_kernel) */
    WG_GEMV_Q8_N = 3,            /* out = W v, 16 rows per lane, 16-byte loads (gemv_q8_n_kernel) */
    WG_GEMV_Q8_ANY_T = 4,        /* out = W^T v element by element: any view */
    WG_GEMV_Q8_ANY_N = 5         /* out = W v element by element: any view */
} wg_gemv_q8_leaf;
typedef struct wg_gemv_q8_plan {
    uint32_t leaf;                           /* wg_gemv_q8_leaf */
    uint32_t rhs_tile, rhs_groups;           /* right-hand sides per pass over the matrix in registers (1, 2, 4, 8); groups of 8 right-hand sides on grid.z */
    uint32_t loads, cols;                    /* WG_GEMV_Q8_T: 16-byte loads in flight per lane and column (a trip is 512 * loads rows) and adjacent columns per half-wave (1 or 4:
                                                they share the vectors' pieces); WG_GEMV_Q8_N: columns in flight per lane, 1 */
    uint32_t nsplit, k_per_split;            /* cut of the contraction over grid.y (1, k: none); no empty split, every boundary a multiple of 16 */
    uint32_t out_per_block;                  /* outputs a workgroup owns: block b takes [b * out_per_block, (b + 1) * out_per_block) */
    uint32_t grid[3], block;                 /* the launch: grid = (output blocks, splits, mats * rhs_groups) */
    uint64_t workspace_bytes;                /* f32 partials of a cut: mats * nsplit * nrhs * outputs * 4 (the context's workspace), 0 without a cut */
    int32_t status;                          /* WG_GEMV_Q8_NOTHING / _UNSUPPORTED */
    char message[128];
} wg_gemv_q8_plan;
/* plan: the plan of `query`. tags (may be NULL): the launch log such a call leaves (the format of wg_debug_take_path), the combine pass of a cut included. */
int wg_debug_gemv_q8_plan(const wg_gemv_q8_query *query, wg_gemv_q8_plan *plan, char *tags, size_t cap);
/* The same for wg_gemv_q4's launcher (gemv_q4_plan.hip). The matrix's sizes and strides count BYTES (two weights each): the contraction length is k = 2 * rows.
 * Sizes and strides of the other operands count f32 elements; *_addr16: the byte address of the view's first element modulo 16. */
typedef struct wg_gemv_q4_query {
    uint32_t trans;                          /* 1: out = W^T v (GemvTr, GemvTrFast), the product there is; 0: out = W v, which the plan refuses */
    uint32_t rows, cols, nrhs, mats;         /* the matrix as stored: rows in BYTES (k / 2) x cols; right-hand sides and matrices (taken from `out`) */
    uint32_t group_rows;                     /* as passed: a positive multiple of 32, or any value >= k */
    uint32_t ldm, lds, ldv, ldo;             /* leading dimensions of m (bytes), scales, v and out */
    uint64_t m_batch, s_batch, v_batch, o_batch; /* matrix strides (m: bytes) */
    uint32_t m_addr16, v_addr16;             /* byte address of the first element of m and of v, modulo 16 (scales and out are reached 4 bytes at a time: any view) */
    uint32_t cus;                            /* compute units of the context's stream */
} wg_gemv_q4_query;
typedef enum wg_gemv_q4_leaf {
    WG_GEMV_Q4_NOTHING = 0,      /* no output element: no launch, WG_OK */
    WG_GEMV_Q4_UNSUPPORTED = 1,  /* no launch: the call returns `status` with `message` */
    WG_GEMV_Q4_T = 2,            /* out = W^T v, a half-wave per column or per 4 adjacent columns, 16-byte loads of 32 weights (gemv_q4_t_kernel) */
    WG_GEMV_Q4_ANY_T = 3         /* out = W^T v a byte (two weights) at a time: any view */
} wg_gemv_q4_leaf;
typedef struct wg_gemv_q4_plan {
    uint32_t leaf;                           /* wg_gemv_q4_leaf */
    uint32_t rhs_tile, rhs_groups;           /* right-hand sides per pass over the matrix in registers (1, 2, 4, 8); groups of 8 right-hand sides on grid.z */
    uint32_t loads, cols;                    /* WG_GEMV_Q4_T: 16-byte loads in flight per lane and column (a trip is 1024 * loads logical rows) and adjacent columns per
                                                half-wave (1 or 4: they share the vectors' pieces) */
    uint32_t nsplit, k_per_split;            /* cut of the contraction over grid.y in LOGICAL rows (1, k: none); no empty split, every boundary a multiple of 1024 */
    uint32_t out_per_block;                  /* outputs a workgroup owns: block b takes [b * out_per_block, (b + 1) * out_per_block) */
    uint32_t grid[3], block;                 /* the launch: grid = (output blocks, splits, mats * rhs_groups) */
    uint64_t workspace_bytes;                /* f32 partials of a cut: mats * nsplit * nrhs * outputs * 4 (the context's workspace), 0 without a cut */
    int32_t status;                          /* WG_GEMV_Q4_NOTHING / _UNSUPPORTED */
    char message[128];
} wg_gemv_q4_plan;
/* plan: the plan of `query`. tags (may be NULL): the launch log such a call leaves (the format of wg_debug_take_path), the combine pass of a cut included. */
int wg_debug_gemv_q4_plan(const wg_gemv_q4_query *query, wg_gemv_q4_plan *plan, char *tags, size_t cap);
/* The same for wg_gemm_q8's launcher (gemm_q8_plan.hip): leaf, column tile, cut of the contraction, grid and workspace bytes as a pure function of the query. Sizes
 * and strides count each operand's own elements (1 byte for `m`, 2 for `x`, 4 for `scales` and `out`); *_addr16: the byte address of the view's first element
 * modulo 16. */
typedef struct wg_gemm_q8_query {
    uint32_t k, outputs, n, mats;            /* contraction length (m.rows), outputs (m.cols), columns of x and out, matrices */
    uint32_t group_rows;                     /* as passed: a positive multiple of 16, or any value >= k */
    uint32_t x_bf16;                         /* x holds bfloat16 (the element name of the tag; no decision reads it) */
    uint32_t ldm, lds, ldx, ldo;             /* leading dimensions of m, scales, x and out */
    uint64_t m_batch, s_batch, x_batch, o_batch; /* matrix strides */
    uint32_t m_addr16, x_addr16, o_addr16;   /* byte address of the first element of m, x and out, modulo 16 (scales are read 4 bytes at a time: any view) */
    uint32_t cus;                            /* compute units of the context's stream */
} wg_gemm_q8_query;
typedef enum wg_gemm_q8_leaf {
    WG_GEMM_Q8_NOTHING = 0,      /* no output element: no launch, WG_OK */
    WG_GEMM_Q8_UNSUPPORTED = 1,  /* no launch: the call returns `status` with `message` */
    WG_GEMM_Q8_MFMA = 2,         /* the streaming kernel: 32 outputs per wave, 16-byte loads, v_mfma_f32_32x32x16_{f16,bf16} (gemm_q8_mfma_kernel) */
    WG_GEMM_Q8_ANY = 3           /* element by element: any view (gemm_q8_any_kernel) */
} wg_gemm_q8_leaf;
typedef struct wg_gemm_q8_plan {
    uint32_t leaf;                           /* wg_gemm_q8_leaf */
    uint32_t col_tiles, col_passes;          /* WG_GEMM_Q8_MFMA: 16-column accumulator tiles per wave (2 or 4: one or two 32 x 32 tiles) and passes over N -- pass i takes
                                                columns [16 col_tiles i, 16 col_tiles (i + 1)) and streams the weights again; WG_GEMM_Q8_ANY: 0, 1 (a wave walks all columns) */
    uint32_t out_per_block;                  /* outputs a workgroup owns: block b takes [b * out_per_block, (b + 1) * out_per_block) */
    uint32_t nsplit, k_per_split;            /* cut of the contraction over grid.y (1, k: none); no empty split, every boundary a multiple of 32 and, where
                                                group_rows < k, of group_rows: a group is never cut */
    uint32_t grid[3], block;                 /* the launch: grid = (output blocks, splits, mats * col_passes) */
    uint64_t workspace_bytes;                /* f32 partials of a cut: mats * nsplit * n * outputs * 4 (the context's workspace), 0 without a cut */
    int32_t status;                          /* WG_GEMM_Q8_NOTHING / _UNSUPPORTED */
    char message[128];
} wg_gemm_q8_plan;
/* plan: the plan of `query`. tags (may be NULL): the launch log such a call leaves (the format of wg_debug_take_path), the combine pass of a cut included. */
int wg_debug_gemm_q8_plan(const wg_gemm_q8_query *query, wg_gemm_q8_plan *plan, char *tags, size_t cap);
/* The same for wg_gemm_q8a8's launcher (gemm_q8a8_plan.hip): wg_gemm_q8_query's fields plus the activations' group size and the view of their scales. Sizes and
 * strides count each operand's own elements (1 byte for `m` and `x`, 4 for `scales`, `x_scales` and `out`); *_addr16: the byte address of the view's first element
 * modulo 16. */
typedef struct wg_gemm_q8a8_query {
    uint32_t k, outputs, n, mats;            /* contraction length (m.rows), outputs (m.cols), columns of x and out, matrices */
    uint32_t group_rows, x_group_rows;       /* as passed: each a positive multiple of 16, or any value >= k; where both are below k one divides the other */
    uint32_t ldm, lds, ldx, ldxs, ldo;       /* leading dimensions of m, scales, x, x_scales and out */
    uint64_t m_batch, s_batch, x_batch, xs_batch, o_batch; /* matrix strides */
    uint32_t m_addr16, x_addr16, o_addr16;   /* byte address of the first element of m, x and out, modulo 16 (the scales are read 4 bytes at a time: any view) */
    uint32_t cus;                            /* compute units of the context's stream */
} wg_gemm_q8a8_query;
typedef enum wg_gemm_q8a8_leaf {
    WG_GEMM_Q8A8_NOTHING = 0,      /* no output element: no launch, WG_OK */
    WG_GEMM_Q8A8_UNSUPPORTED = 1,  /* no launch: the call returns `status` with `message` */
    WG_GEMM_Q8A8_MFMA = 2,         /* the streaming kernel: 32 outputs per wave, 16-byte loads of both operands, v_mfma_i32_32x32x32_i8 (gemm_q8a8_mfma_kernel) */
    WG_GEMM_Q8A8_ANY = 3           /* element by element: any view (gemm_q8a8_any_kernel) */
} wg_gemm_q8a8_leaf;
typedef struct wg_gemm_q8a8_plan {
    uint32_t leaf;                           /* wg_gemm_q8a8_leaf */
    uint32_t col_tiles, col_passes;          /* WG_GEMM_Q8A8_MFMA: 16-column accumulator tiles per wave (2 or 4: one or two 32 x 32 tiles) and passes over N -- pass i takes
                                                columns [16 col_tiles i, 16 col_tiles (i + 1)) and streams the weights again; WG_GEMM_Q8A8_ANY: 0, 1 (a wave walks all columns) */
    uint32_t out_per_block;                  /* outputs a workgroup owns: block b takes [b * out_per_block, (b + 1) * out_per_block) */
    uint32_t nsplit, k_per_split;            /* cut of the contraction over grid.y (1, k: none); no empty split; every boundary is a CHAIN boundary: a multiple of 32, of
                                                whichever group sizes are below k and, where neither is, of 1024 */
    uint32_t grid[3], block;                 /* the launch: grid = (output blocks, splits, mats * col_passes) */
    uint64_t workspace_bytes;                /* f32 partials of a cut: mats * nsplit * n * outputs * 4 (the context's workspace), 0 without a cut */
    int32_t status;                          /* WG_GEMM_Q8A8_NOTHING / _UNSUPPORTED */
    char message[128];
} wg_gemm_q8a8_plan;
/* plan: the plan of `query`. tags (may be NULL): the launch log such a call leaves (the format of wg_debug_take_path), the combine pass of a cut included. */
int wg_debug_gemm_q8a8_plan(const wg_gemm_q8a8_query *query, wg_gemm_q8a8_plan *plan, char *tags, size_t cap);
/* The choice of wg_quantize_q8's launcher (quantize_q8.hip) as a pure function of the query: leaf, block and grid. Strides count each operand's own elements;
 * *_addr16: the byte address of the view's first element modulo 16; src_elem: bytes per source element (4 or 2). */
typedef struct wg_quantize_q8_query {
    uint32_t rows, cols, mats, group_rows, src_elem;
    uint32_t ldq, ldsrc;
    uint64_t q_batch, src_batch;
    uint32_t q_addr16, src_addr16;
} wg_quantize_q8_query;
typedef enum wg_quantize_q8_leaf {
    WG_QUANTIZE_Q8_NOTHING = 0,      /* no element: no launch, WG_OK */
    WG_QUANTIZE_Q8_UNSUPPORTED = 1,  /* no launch: the call returns `status` with `message` */
    WG_QUANTIZE_Q8_VEC = 2,          /* a lane per 16 rows: 16-byte loads and one 16-byte store, the max over the group_rows / 16 lanes of a group by cross-lane exchange */
    WG_QUANTIZE_Q8_ANY = 3           /* a wave or a workgroup per (group, column) in two sweeps, element by element: any view */
} wg_quantize_q8_leaf;
typedef struct wg_quantize_q8_plan {
    uint32_t leaf;                           /* wg_quantize_q8_leaf */
    uint32_t group_lanes;                    /* VEC: lanes that share a group (group_rows / 16: a power of two, 2 .. 64) */
    uint32_t blocks_per_col;                 /* grid.x = blocks_per_col * cols: VEC -- workgroups of 256 lanes per column; ANY -- groups per column */
    uint32_t grid[3], block;                 /* the launch: grid = (blocks_per_col * cols, 1, mats); ANY: 64 threads up to 1024 rows per group, else 256 */
    int32_t status;
    char message[128];
} wg_quantize_q8_plan;
int wg_debug_quantize_q8_plan(const wg_quantize_q8_query *query, wg_quantize_q8_plan *plan);
/* The same for wg_gemm_q4's launcher (gemm_q4_plan.hip). `k` counts LOGICAL rows (k = 2 * m.rows); ldm and m_batch count BYTES of the packed matrix; the other
 * operands count their own elements (2 bytes for `x`, 4 for `scales` and `out`); *_addr16: the byte address of the view's first element modulo 16. */
typedef struct wg_gemm_q4_query {
    uint32_t k, outputs, n, mats;            /* contraction length in logical rows (2 * m.rows), outputs (m.cols), columns of x and out, matrices */
    uint32_t group_rows;                     /* as passed: a positive multiple of 32, or any value >= k */
    uint32_t x_bf16;                         /* x holds bfloat16 (the element name of the tag; no decision reads it) */
    uint32_t ldm, lds, ldx, ldo;             /* leading dimensions of m (bytes), scales, x and out */
    uint64_t m_batch, s_batch, x_batch, o_batch; /* matrix strides (m: bytes) */
    uint32_t m_addr16, x_addr16, o_addr16;   /* byte address of the first element of m, x and out, modulo 16 (scales are read 4 bytes at a time: any view) */
    uint32_t cus;                            /* compute units of the context's stream */
} wg_gemm_q4_query;
typedef enum wg_gemm_q4_leaf {
    WG_GEMM_Q4_NOTHING = 0,      /* no output element: no launch, WG_OK */
    WG_GEMM_Q4_UNSUPPORTED = 1,  /* no launch: the call returns `status` with `message` */
    WG_GEMM_Q4_MFMA = 2,         /* the streaming kernel: 32 outputs per wave, 16-byte loads of 32 weights, v_mfma_f32_32x32x16_{f16,bf16} (gemm_q4_mfma_kernel) */
    WG_GEMM_Q4_ANY = 3           /* element by element, a byte (two weights) per lane and step: any view (gemm_q4_any_kernel) */
} wg_gemm_q4_leaf;
typedef struct wg_gemm_q4_plan {
    uint32_t leaf;                           /* wg_gemm_q4_leaf */
    uint32_t step;                           /* logical rows of one step of the streaming kernel: 32. k % step == 0 is its condition, and step divides every cut */
    uint32_t col_tiles, col_passes;          /* WG_GEMM_Q4_MFMA: 16-column accumulator tiles per wave (2 or 4: one or two 32 x 32 tiles) and passes over N -- pass i takes
                                                columns [16 col_tiles i, 16 col_tiles (i + 1)) and streams the weights again; WG_GEMM_Q4_ANY: 0, 1 (a wave walks all columns) */
    uint32_t out_per_block;                  /* outputs a workgroup owns: block b takes [b * out_per_block, (b + 1) * out_per_block) */
    uint32_t nsplit, k_per_split;            /* cut of the contraction over grid.y in LOGICAL rows (1, k: none); no empty split, every boundary a multiple of 32 and,
                                                where group_rows < k, of group_rows: a group is never cut */
    uint32_t grid[3], block;                 /* the launch: grid = (output blocks, splits, mats * col_passes) */
    uint64_t workspace_bytes;                /* f32 partials of a cut: mats * nsplit * n * outputs * 4 (the context's workspace), 0 without a cut */
    int32_t status;                          /* WG_GEMM_Q4_NOTHING / _UNSUPPORTED */
    char message[128];
} wg_gemm_q4_plan;
/* plan: the plan of `query`. tags (may be NULL): the launch log such a call leaves (the format of wg_debug_take_path), the combine pass of a cut included. */
int wg_debug_gemm_q4_plan(const wg_gemm_q4_query *query, wg_gemm_q4_plan *plan, char *tags, size_t cap);
/* The same for the launcher of wg_gemv, wg_gemv_mixed and the fused wg_gemv_reduce (gemv_plan.hip): leaf, right-hand-side tile, cut of the contraction, grids and
 * workspace bytes as a pure function of the query. The query describes the call as the vec4 kernels get it (api.hip: the views as they are, or their staged copies);
 * sizes and strides count each operand's own elements. */
typedef struct wg_gemv_query {
    uint32_t trans;                          /* 0: out = m v (m is rows_out x k); 1: out = m^T v (m is k x rows_out) */
    uint32_t rows_out, k, nrhs, nmats;       /* outputs per vector, contraction length, right-hand sides, matrices */
    uint32_t m_elem, v_elem;                 /* bytes per element of the matrix and of the vectors / the result: 2 or 4 (wg_gemv_mixed: 2 and 4) */
    uint32_t bf16;                           /* the 16-bit elements are bfloat16 (the element prefix of the tags; no decision reads it) */
    uint32_t gemm16;                         /* the 16-bit-both form (wg_gemv on f16 / bf16): the call may be handed to the 16-bit Gemm kernels */
    uint32_t ldm, ldv, ldo;                  /* leading dimensions of m, v and out (out's, and its matrix stride, are part of the call; no decision reads them yet) */
    uint64_t m_batch, v_batch, o_batch;      /* matrix strides */
    uint32_t m_addr16, v_addr16;             /* byte address of the first element of m and v, modulo 16 (the 16-byte loads of gemv.tcols/e=8) */
    uint32_t cus;                            /* compute units of the context's stream */
    int32_t gemvt_lds;                       /* WG_TUNE_GEMVT_LDS */
} wg_gemv_query;
typedef enum wg_gemv_leaf {
    WG_GEMV_NOTHING = 0,        /* no output element: no launch, WG_OK */
    WG_GEMV_UNSUPPORTED = 1,    /* no launch: the call returns `status` with `message` */
    WG_GEMV_SMALL = 2,          /* out = m v, launch-bound: one kernel, no partials (gemv_n_small_kernel); the calls the fused Gemv + Reduce takes */
    WG_GEMV_N = 3,              /* out = m v (gemv_n_kernel) */
    WG_GEMV_T = 4,              /* out = m^T v, 4 columns per wave (gemv_t_kernel) */
    WG_GEMV_TCOLS = 5,          /* out = m^T v, a half-wave per column, 1 or 2 vectors (gemv_t_cols_kernel) */
    WG_GEMV_TLDS = 6,           /* f32 out = m^T v, 2 .. 8 vectors held in the LDS (gemv_t_lds_kernel) */
    WG_GEMV_AS_GEMM32 = 7,      /* handed to the f32 few-column Gemm kernel: `gemm32` is that call's plan */
    WG_GEMV_AS_GEMM16 = 8       /* handed to the 16-bit Gemm launcher, which plans the call itself (gemm16_plan.hip) */
} wg_gemv_leaf;
typedef struct wg_gemv_plan {
    uint32_t leaf;                           /* wg_gemv_leaf */
    uint32_t rhs_tile, rhs_groups;           /* right-hand sides per pass over the matrix in registers (1, 2, 4, 8); groups of 8 right-hand sides on grid.z */
    uint32_t e, u, v;                        /* WG_GEMV_TCOLS: elements per load (4, or 8: one 16-byte load of 16-bit elements), loads in flight per lane, vectors (1, 2) */
    uint32_t rl;                             /* WG_GEMV_SMALL: lanes x float4 of rows per workgroup (2, 4, 8) */
    uint32_t lds_cols, lds_threads;          /* WG_GEMV_TLDS: adjacent columns per half-wave, threads per workgroup, ... */
    uint32_t lds_kc, lds_bytes;              /* ... contracted rows per LDS chunk (k: one chunk) and the dynamic LDS of a workgroup */
    uint32_t nsplit, k_per_split;            /* cut of the contraction over grid.y (1, k: none), final: no empty split, every boundary a multiple of 4 */
    uint32_t grid[3], block;                 /* the launch */
    uint32_t combine_grid[3];                /* nsplit > 1: the pass that sums the partials (256 threads) */
    uint64_t workspace_bytes;                /* f32 partials of a cut: nmats * nsplit * nrhs * rows_out * 4 (the context's workspace), 0 without a cut */
    int32_t status;                          /* WG_GEMV_NOTHING / _UNSUPPORTED */
    char message[128];
    wg_gemm32_plan gemm32;                   /* WG_GEMV_AS_GEMM32 */
} wg_gemv_plan;
/* plan: the plan of `query`. tags (may be NULL): the launch log such a call leaves (the format of wg_debug_take_path) from "gemv>" on: the element prefix
 * ("f32.gemv", "f16.gemv", "bf16.gemv", "f16w.gemv", "bf16w.gemv") where the launcher logs one, the leaf and the combine pass; for WG_GEMV_AS_GEMM32 the tags of the
 * few-column plan; for WG_GEMV_AS_GEMM16 "gemv>" alone (what follows is wg_debug_gemm16_plan's). */
int wg_debug_gemv_plan(const wg_gemv_query *query, wg_gemv_plan *plan, char *tags, size_t cap);
/* ... and for the any-alignment kernels (gemv_any.hip) on the same query (it reads trans, rows_out, k, nrhs, nmats, m_elem and cus): the (matrix, right-hand side)
 * pairs go over grid.z in chunks of `zchunk`, each with its own combine pass. */
typedef struct wg_gemv_any_plan {
    uint32_t launch;                         /* 0: nothing to do (status WG_OK) or refused (`status`, `message`) */
    uint32_t nsplit, per_split;              /* cut of the contraction over grid.y: whole 64-column chunks (N) / whole 64-lane row steps (T) per split */
    uint32_t grid_x, zchunk, nchunks;        /* output blocks; pairs per launch (<= 65535) and launches */
    uint32_t nt;                             /* the matrix is read with the non-temporal hint */
    uint64_t workspace_bytes;                /* f32 partials of one chunk: zchunk * nsplit * rows_out * 4, 0 without a cut */
    int32_t status;
    char message[128];
    char tag[48];                            /* "gemv_any/n,ns=4", "gemv_any/t,ns=1,chunks=2" */
} wg_gemv_any_plan;
int wg_debug_gemv_any_plan(const wg_gemv_query *query, wg_gemv_any_plan *plan, char *tags, size_t cap);
int wg_ctx_get_tuning(const wg_ctx *ctx, wg_tuning key, int *value);
/* Diagnostics / tests (no context, no device): the predicate behind WG_ERR_ALIASED. Returns 1 when the footprints of two views share a byte, 0 when they do not.
 * byte_base_*: the byte address of element 0 of the buffer each view indexes (wg_buf_device_ptr; any integers do, only their difference matters); elem_size: bytes
 * per element (both views). A view with a zero size overlaps nothing. Disjoint byte intervals are answered at once; intersecting intervals are decided exactly by
 * walking column runs (one per column and matrix; columns that touch and matrices that touch are folded first, so dense views are one run) while the two views
 * have at most WG_VIEWS_OVERLAP_MAX_RUNS runs between them; above that the answer is 1 whatever the truth. *exact (may be NULL) = 0 for such a conservative
 * answer, 1 otherwise. The answer is never 0 for footprints that intersect. */
#define WG_VIEWS_OVERLAP_MAX_RUNS 4096
int wg_debug_views_overlap(wg_view_shape shape_a, uint64_t byte_base_a, wg_view_shape shape_b, uint64_t byte_base_b, uint32_t elem_size, int *exact);

/* Pre-size the context's scratch (GEMV split-K partials) so that no operator allocates while recording. An operator that would
 * have to grow a scratch region inside a recording returns WG_ERR_WORKSPACE. Scratch regions that a live command buffer may
 * replay into are never freed before that command buffer is destroyed. */
int wg_ctx_reserve_workspace(wg_ctx *ctx, size_t bytes);

/* ------------------------------------------------------------------------------------------------ */
/* buffers  (TensorBuilder::build / build_init / build_bytes, tensor.rs:115-186)                     */
/* ------------------------------------------------------------------------------------------------ */
/* Uninitialised buffer of `bytes` bytes (0 is legal: an empty tensor). */
int wg_buf_create(wg_ctx *ctx, size_t bytes, uint32_t usage, wg_buf **out);
/* create_buffer_init: allocate and upload synchronously (tensor.rs:149-161). */
int wg_buf_create_init(wg_ctx *ctx, const void *data, size_t bytes, uint32_t usage, wg_buf **out);
/* Non-owning wrapper around device memory someone else allocated (e.g. a torch tensor's data_ptr()). */
int wg_buf_wrap(wg_ctx *ctx, void *device_ptr, size_t bytes, wg_buf **out);
int wg_buf_destroy(wg_buf *buf); /* Drop for GpuTensor / Buffer */
size_t wg_buf_size(const wg_buf *buf);
void *wg_buf_device_ptr(const wg_buf *buf);
/* Queue::write_buffer: stream-ordered host->device copy of `bytes` at byte `offset`. Host memory may be pageable. */
int wg_buf_write(wg_ctx *ctx, wg_buf *dst, size_t offset, const void *data, size_t bytes);
/* GpuTensor::read / read_to (tensor.rs:300-384): device->host, BLOCKS until the data is in `dst`. */
int wg_buf_read(wg_ctx *ctx, const wg_buf *src, size_t offset, void *dst, size_t bytes);
/* CommandEncoder::copy_buffer_to_buffer (tensor.rs:227-264): stream-ordered device copy. */
int wg_buf_copy(wg_ctx *ctx, const wg_buf *src, size_t src_offset, wg_buf *dst, size_t dst_offset, size_t bytes);
int wg_buf_fill_zero(wg_ctx *ctx, wg_buf *buf);

/* ------------------------------------------------------------------------------------------------ */
/* operators                                                                                         */
/* ------------------------------------------------------------------------------------------------ */
/*
 * Gemm::dispatch_generic (wgebra gemm.rs:65-127): out = m1 * m2 (WG_GEMM, WG_GEMM_FAST) or m1^T * m2
 * (WG_GEMM_TR, WG_GEMM_TR_FAST), batched over size[2]; `out` is overwritten.
 *   DIM_MISMATCH  : the five assert_eq! of gemm.rs:91-95.
 *   Views that are not vec4-aligned (rows / stride / stride_mat / offset of a view, or M, N, K, not a multiple of 4 -- what
 *                   GpuMatrix::slice / rows / column hand out for odd offsets and lengths, tensor.rs:574-626): the reference's
 *                   kernels bind array<vec4<f32>> and address the wrong elements there (shape.wgsl:64-66). Here they compute
 *                   op(m1) m2 like any other view. Any offset / stride runs on the tuned kernels as it is (16-byte accesses and LDS-DMA take
 *                   element-aligned addresses on this target); lengths that are not multiples of 4 (of M and K; N too for f32 products with up to 128 rows -- otherwise any N runs as it is)
 *                   are staged into dense zero-padded copies of the operands that carry them (HBM-bound passes in a context scratch that cannot grow
 *                   inside a recording: WG_ERR_WORKSPACE); 1 .. 7 columns on otherwise aligned views run as a Gemv with that many right-hand
 *                   sides, without any copy. Only a view that exceeds its buffer is an error.
 *   *_FAST        : the reference requires K % 256 == 0 and reads out of bounds otherwise (gemm.wgsl:40,162);
 *                   here every K % 4 == 0 is accepted and all four variants run the same tuned kernel.
 * dtype WG_F16 (extension): f16 operands, f32 accumulation, result rounded once (RNE) to f16. WG_BF16 (extension): likewise on bfloat16 operands (wg_dtype).
 *   ALIASED       : `out` shares a byte with `m1` or with `m2` (the aliasing rule, top of this file). `m1` and `m2` may overlap each other: both are only read.
 */
int wg_gemm(wg_ctx *ctx, wg_gemm_variant variant, wg_dtype dtype,
            wg_buf *out, wg_view_shape out_shape,
            const wg_buf *m1, wg_view_shape m1_shape,
            const wg_buf *m2, wg_view_shape m2_shape);

/*
 * Extension: BLAS-style update  out = alpha * op(m1) * m2 + beta * out.  Same views, checks and variants as
 * wg_gemm; beta == 0 never reads `out` (NaN/Inf there are overwritten, like wg_gemm), and (alpha, beta) = (1, 0) is
 * bit-identical to wg_gemm. alpha, beta are f32 for every dtype; f16 and bf16: alpha*acc + beta*c is formed in f32 and rounded once.
 * ALIASED: `out` overlapping `m1` or `m2` (the aliasing rule) -- reading `out` itself for beta != 0 is the update, not an alias.
 */
int wg_gemm_ex(wg_ctx *ctx, wg_gemm_variant variant, wg_dtype dtype, float alpha, float beta,
               wg_buf *out, wg_view_shape out_shape,
               const wg_buf *m1, wg_view_shape m1_shape,
               const wg_buf *m2, wg_view_shape m2_shape);

/*
 * Gemv::dispatch_generic (wgebra gemv.rs:64-137): out[:,y,z] = m[:,:,z] * v[:,y,z] (or m^T), for every RHS
 * column y < out.size[1] and matrix z < out.size[2]; `out` is overwritten.
 *   DIM_MISMATCH  : gemv.rs:89-90 (only m_cols == v_rows and m_rows == out_rows are checked there too).
 *   PRECONDITION  : WG_GEMV_FAST / WG_GEMV_TR_FAST with out rows % 4 != 0 (assert_eq! gemv.rs:122). Views that are not
 *                   vec4-aligned run on the matrix where it lies, one pass over it per right-hand side (gemv_any.hip: 16-byte loads at
 *                   element-aligned addresses).
 *   WG_GEMV_TR_FAST with m rows % 128 != 0 silently runs as WG_GEMV_TR (gemv.rs:99-104) -- same kernel here.
 * dtype WG_F16 (extension): f16 elements, f32 accumulation, one rounding at the store -- the same HBM-bound kernels. WG_BF16 (extension): likewise on bfloat16 elements.
 * Several right-hand sides: one pass over the matrix for all of them; from 9 on -- and from 3 on when the matrix is past the launch-bound
 * sizes -- that pass runs on the Gemm kernels (same contract: f32 accumulation, results within the Gemv tolerance, deterministic).
 *   ALIASED       : `out` shares a byte with the part of `m` or of `v` the call addresses (the aliasing rule; e.g. `out` = a column of `m`).
 */
int wg_gemv(wg_ctx *ctx, wg_gemv_variant variant, wg_dtype dtype,
            wg_buf *out, wg_view_shape out_shape,
            const wg_buf *m, wg_view_shape m_shape,
            const wg_buf *v, wg_view_shape v_shape);

/*
 * Extension: mixed-precision Gemv -- a 16-bit matrix, f32 vectors and an f32 result (the decode step of an inference stack: weights stored in f16 / bf16,
 * activations kept in f32). `m` holds m_dtype elements (WG_F16 or WG_BF16); `v` and `out` hold f32; every view shape counts elements of its own operand's type,
 * and the bounds checks use each operand's own element size. m_dtype == WG_F32 forwards to wg_gemv(.., WG_F32, ..) unchanged (a caller generic over the weight
 * type needs no branch). Everything else is wg_gemv's contract, with its status codes and messages: the two dimension checks, *_FAST with out rows % 4 != 0
 * (PRECONDITION), WG_GEMV_TR_FAST falling back to WG_GEMV_TR, zero-sized buffers / views skipped with WG_OK, right-hand sides and batch taken from `out`.
 * Arithmetic:
 *   - matrix elements are widened exactly; `v` is read as the f32 it is and never narrowed; products and sums are f32 FMAs; the result is stored as the f32
 *     accumulator -- there is no rounding step;
 *   - `out` is overwritten (NaN / Inf already in it do not survive); an Inf or NaN in the last valid column or row of `m` reaches only the results the
 *     mathematics says it reaches (load slots past the end contribute an exact zero);
 *   - deterministic: no atomics, a fixed summation order -- two calls give identical bits;
 *   - the kernels and the summation order are those the 16-bit wg_gemv picks for the same shape, views and context (the plan is made with the MATRIX's
 *     element size): while that call stays on the Gemv kernels the accumulators are the same bit for bit, and one round-to-nearest-even of this call's result
 *     reproduces its result whenever `v` is representable in the 16-bit type.
 * Right-hand sides: this call NEVER takes the Gemm kernels (they would round `v` to 16 bits). Up to 8 right-hand sides share one pass over the matrix; more
 * run as groups of 8 on the Gemv kernels, one pass over the matrix per group. nmats * ceil(nrhs / 8) > 65535 is WG_ERR_UNSUPPORTED.
 * Views that are not vec4-aligned, per operand as in wg_gemv: a matrix that is off (offset, leading dimension, lengths) runs where it lies (gemv_any.hip's
 * mixed instances); vectors or an `out` that are off are staged as f32 copies in a context scratch that cannot grow inside a recording (WG_ERR_WORKSPACE).
 *   ALIASED       : `out` shares a byte with the part of `m` or of `v` the call addresses -- on addresses, so `out` and `m` may live in one buffer although
 *                   their element sizes differ (compared in 2-byte units, with the bound of the aliasing rule).
 * wg_debug_take_path: the element prefix is "f16w.gemv" / "bf16w.gemv" (w: 16-bit weights only), followed by the dtype-free tags of wg_gemv.
 */
int wg_gemv_mixed(wg_ctx *ctx, wg_gemv_variant variant, wg_dtype m_dtype,
                  wg_buf *out, wg_view_shape out_shape,
                  const wg_buf *m, wg_view_shape m_shape,
                  const wg_buf *v, wg_view_shape v_shape);

/*
 * Extension: Gemv on 8-bit weights with group scales -- an int8_t matrix, f32 scales, f32 vectors and an f32 result (the decode step on weights stored as in Q8_0 or
 * per-channel int8: half the bytes of the 16-bit wg_gemv_mixed). The matrix is W[r, c, z] = scales[r / G, c, z] * (float)m[r, c, z] with G = group_rows: groups run
 * along the matrix's ROWS, the contiguous dimension, for every variant (GemvTr on weights stored k x outputs: a group is group_rows consecutive weights of one
 * output). out = W v (WG_GEMV, WG_GEMV_FAST) or W^T v (WG_GEMV_TR, WG_GEMV_TR_FAST), for every right-hand side and matrix of `out`; no alpha, no beta: wg_gemv's product.
 * `m` holds int8_t (all 256 values are legal, -128 included), column-major like every view; `scales` holds f32, ceil(m.rows / group_rows) x m.cols x m.mats; `v` and
 * `out` hold f32. Every view shape counts elements of its own operand's type; the bounds checks use 1 byte for `m` and 4 bytes for the others. wg_dtype has no 8-bit
 * value and gets none: no other entry point reads 1-byte elements.
 *   group_rows    : a positive multiple of 16, or any positive value >= m.rows (one scale per column: `scales` has one row). Anything else is WG_ERR_INVALID_ARG.
 *   DIM_MISMATCH  : wg_gemv's two checks with its message; then `scales` of another shape than the one above ("Gemv: dimension mismatch. (m [..], group_rows G,
 *                   scales [..], expected [..])").
 * Everything else is wg_gemv_mixed's contract, in its order, with its status codes and messages: the NULL context ("Gemv: ctx is NULL"), NULL buffers, the unknown
 * variant, *_FAST with out rows % 4 != 0 (PRECONDITION), WG_GEMV_TR_FAST falling back to WG_GEMV_TR, zero-sized buffers / views skipped with WG_OK, right-hand sides
 * and batch taken from `out`, views that exceed their buffer, nmats * ceil(nrhs / 8) > 65535 (UNSUPPORTED), WG_ERR_WORKSPACE when the partials of a cut contraction
 * would have to grow the context's workspace inside a recording.
 * Arithmetic:
 *   - int8 is widened exactly; `v` and `scales` are read as the f32 they are and never narrowed; every operation is an f32 FMA or multiply; the f32 accumulator is
 *     stored as it is. Nothing is flushed: subnormal scales, vector entries and results are kept.
 *   - where the scale enters (the kernel's choice; each of the k terms takes at most two f32 roundings either way):
 *       GemvTr, aligned views (gemv_q8_t_kernel): per 16-weight PIECE -- d = sum of the piece's 16 products q * v (sequential FMAs from zero), then
 *         acc = fmaf(scale, d, acc). A piece never straddles a group. The unscaled d must be finite for a finite result (|q| <= 128: no concern below 1e35);
 *       Gemv, aligned views (gemv_q8_n_kernel): per column and 16-row piece into the VECTOR entry -- t = scale * v[c], then acc[r] = fmaf(q, t, acc[r]);
 *       any other view (the element-by-element kernels): per ELEMENT -- w = scale * q (the dequantised weight), then acc = fmaf(w, v, acc).
 *   - Inf and NaN behave as in the f32 product of the dequantised matrix with `v`: 0 * Inf is NaN (a zero scale against an Inf in `v`, a zero weight against it),
 *     and a NaN reaches exactly the outputs whose sums contain it; load slots past the end of a range contribute nothing. `out` is overwritten.
 *   - deterministic: no atomics; a cut contraction writes f32 partials that one pass adds in a fixed order -- two calls give identical bits.
 * Which kernels (gemv_q8_plan.hip, wg_debug_gemv_q8_plan): the two streaming kernels take views where m.rows % 16 == 0, the matrix's first element, leading dimension
 * and matrix stride are multiples of 16 bytes, and the operand the kernel reaches with float4 accesses -- `v` for GemvTr, `out` for Gemv -- is vec4-aligned (address, leading
 * dimension and matrix stride multiples of 16 bytes where they count; the other one is reached one float at a time and may be any view); every other view runs where it lies on the element-by-element kernels -- correct, not fast, and without any copy of the matrix. Up to 8 right-hand sides share one
 * pass over the matrix; more run as groups of 8 on grid.z.
 *   ALIASED       : `out` shares a byte with the part of `m`, of `scales` or of `v` the call addresses -- on addresses, `out` against `m` in 1-byte units, so both may
 *                   live in one buffer: touching is legal, one shared byte is refused. The read operands may overlap each other.
 * wg_debug_take_path: tags begin "gemv_q8/": "gemv_q8/t,nr=1,u=2,c=4,ns=1" (right-hand-side tile, loads in flight per column, columns per half-wave, splits), "gemv_q8/n,nr=8,u=8,ns=4", "gemv_q8/combine,ns=4", "gemv_q8/any_t", "gemv_q8/any_n".
 */
int wg_gemv_q8(wg_ctx *ctx, wg_gemv_variant variant, uint32_t group_rows,
               wg_buf *out, wg_view_shape out_shape,             /* f32 */
               const wg_buf *m, wg_view_shape m_shape,           /* int8_t, column-major like every view */
               const wg_buf *scales, wg_view_shape scales_shape, /* f32: ceil(m.rows / group_rows) x m.cols x mats */
               const wg_buf *v, wg_view_shape v_shape);          /* f32 */

/*
 * Extension: GemvTr on packed 4-bit weights with group scales -- the decode product on weights stored as in Q4_0, or GPTQ / AWQ without zero points: half the bytes
 * of wg_gemv_q8. out = W^T v, for every right-hand side and matrix of `out`; no alpha, no beta.
 * The operand: `m` holds packed BYTES, column-major like every view. Byte j of a column holds logical row 2 j in its LOW nibble and row 2 j + 1 in its HIGH nibble. A
 * nibble n in 0 .. 15 stands for the integer q = n - 8, so q is in -8 .. 7 and all 16 values are legal. W[r, c, z] = scales[r / G, c, z] * (float)q[r, c, z] with
 * G = group_rows: one f32 scale per G consecutive LOGICAL rows of a column; groups run along the contraction, as in wg_gemv_q8. m_shape counts BYTES: rows, leading
 * dimension, offset and matrix stride. The contraction length is k = 2 * m.rows. `scales` holds f32, ceil(k / G) x m.cols x mats; `v` holds f32 with k rows; `out`
 * holds f32 with m.cols rows. Right-hand sides and matrices are taken from `out`. The bounds checks use 1 byte for `m` and 4 bytes for the others. Scales stay in a
 * tensor of their own, as for wg_gemv_q8: repacking another container's block layout is a host permutation and not part of this call. wg_dtype has no 4-bit value
 * and gets none.
 *   variant       : WG_GEMV_TR is the product above; WG_GEMV_TR_FAST is the same call. WG_GEMV and WG_GEMV_FAST would put the groups and the nibble pairs along the
 *                   outputs, a layout nobody stores: WG_ERR_UNSUPPORTED ("... wg_gemv_q8 computes out = W v ..."). The refusal comes right behind the checks of
 *                   the context, the buffers and the variant's range, BEFORE any dimension, group_rows or size is looked at: a mismatched or a zero-sized call
 *                   with these variants is WG_ERR_UNSUPPORTED too, not WG_ERR_DIM_MISMATCH or WG_OK (wg_gemm_q8's refused out = W x does the same).
 *   group_rows    : a positive multiple of 32, or any positive value >= k (one scale per output: `scales` has one row). Anything else is WG_ERR_INVALID_ARG.
 *   DIM_MISMATCH  : v.rows != 2 * m.rows or out.rows != m.cols ("Gemv: dimension mismatch. (out [..], m [..]^T packed: k K, v [..])"); then `scales` of another shape
 *                   than the one above ("Gemv: dimension mismatch. (m [..] packed: k K, group_rows G, scales [..], expected [..])").
 * Everything else is wg_gemv_q8's contract, in its order, with its status codes and messages: the NULL context ("Gemv: ctx is NULL"), NULL buffers, the unknown
 * variant, zero-sized buffers / views skipped with WG_OK, views that exceed their buffer, nmats * ceil(nrhs / 8) > 65535 (UNSUPPORTED), WG_ERR_WORKSPACE when the
 * partials of a cut contraction would have to grow the context's workspace inside a recording.
 * Arithmetic:
 *   - q = n - 8 is formed exactly (an f32 integer) before anything is multiplied: the -8 is NOT folded into a per-piece correction (sum n v - 8 sum v would leave
 *     rounding residue of the size of 8 |s v| under a zero weight). `v` and `scales` are read as the f32 they are and never narrowed; every operation is an f32 FMA
 *     or multiply; the f32 accumulator is stored as it is. Nothing is flushed: subnormal scales, vector entries and results are kept.
 *   - where the scale enters (each of the k terms takes at most two f32 roundings either way):
 *       aligned views (gemv_q4_t_kernel): per PIECE of 16 weights -- half a 16-byte load, logical rows 16 i .. 16 i + 15 --: d = the piece's 16 products q * v
 *         summed by sequential FMAs from zero in row order, then acc = fmaf(scale, d, acc). A piece never straddles a group. The unscaled d must be finite for a
 *         finite result (|q| <= 8: no concern below 1e36);
 *       any other view (gemv_q4_any_t_kernel): per ELEMENT -- w = scale * q (the dequantised weight), then acc = fmaf(w, v, acc).
 *   - Inf and NaN behave as in the f32 product of the dequantised matrix with `v`: 0 * Inf is NaN (a zero scale against an Inf in `v`, a zero weight against it), and
 *     a NaN reaches exactly the outputs whose sums contain it; load slots past the end of a range contribute nothing. `out` is overwritten.
 *   - deterministic: no atomics; a cut contraction writes f32 partials that one pass adds in a fixed order -- two calls give identical bits.
 * Which kernels (gemv_q4_plan.hip, wg_debug_gemv_q4_plan): the streaming kernel takes views where m.rows % 16 == 0 (k % 32 == 0), the matrix's first byte, leading
 * dimension and matrix stride are multiples of 16 bytes, and `v` is vec4-aligned (address, leading dimension and matrix stride multiples of 16 bytes where they
 * count); `scales` and `out` are reached one float at a time and may be any view. Every other view runs where it lies on the element-by-element kernel -- correct,
 * not fast, and without any copy of the matrix. Up to 8 right-hand sides share one pass over the matrix; more run as groups of 8 on grid.z.
 *   ALIASED       : `out` shares a byte with the part of `m`, of `scales` or of `v` the call addresses -- on addresses, `out` against `m` in 1-byte units, so both may
 *                   live in one buffer: touching is legal, one shared byte is refused. The read operands may overlap each other.
 * wg_debug_take_path: tags begin "gemv_q4/": "gemv_q4/t,nr=1,u=2,c=4,ns=1" (right-hand-side tile, loads in flight per column, columns per half-wave, splits),
 * "gemv_q4/combine,ns=4", "gemv_q4/any_t".
 */
int wg_gemv_q4(wg_ctx *ctx, wg_gemv_variant variant, uint32_t group_rows,
               wg_buf *out, wg_view_shape out_shape,             /* f32: m.cols rows */
               const wg_buf *m, wg_view_shape m_shape,           /* packed bytes, two weights each: k / 2 x outputs x mats, column-major */
               const wg_buf *scales, wg_view_shape scales_shape, /* f32: ceil(k / group_rows) x m.cols x mats */
               const wg_buf *v, wg_view_shape v_shape);          /* f32: k = 2 * m.rows rows */

/*
 * Extension: Gemm on 16-bit operands with an f32 result -- out = alpha * op(m1) * m2 + beta * out with the f32 accumulators of the matrix cores stored as they
 * are (a result past the f16 range, a K-chunked or residual accumulation through beta that is not re-rounded at every step, the prefill counterpart of
 * wg_gemv_mixed). `m1` and `m2` hold in_dtype elements (WG_F16 or WG_BF16); `out` holds f32; every view shape counts elements of its own operand's type, and the
 * bounds checks use each operand's own element size (an `out` buffer sized for 2-byte elements is refused as exceeding its buffer). in_dtype == WG_F32 forwards
 * to wg_gemm_ex(.., WG_F32, ..) unchanged (a caller generic over the operand type needs no branch). Everything else is wg_gemm_ex's contract, with its status
 * codes and messages: the dimension check, unknown variant, zero-sized buffers / views skipped with WG_OK, views that exceed their buffer; WG_ERR_WORKSPACE inside
 * a recording when a padding or staging scratch would have to grow.
 * Arithmetic:
 *   - operands are widened exactly; the f32 accumulator is that of the 16-bit wg_gemm_ex on the same leaf -- the same MFMA chain in the same order;
 *   - r = alpha * acc is rounded to f32 (skipped for alpha == 1), then r = fmaf(beta, c, r) with c read as the f32 it is; beta == 0 never reads `out` (NaN / Inf
 *     there are overwritten); r is stored as it is -- there is no 16-bit rounding anywhere;
 *   - deterministic: no atomics, K cuts are added in ascending order;
 *   - same leaf, same accumulator: while this call and the 16-bit call for the same shape, views, knobs and context log the same leaf, one round-to-nearest-even
 *     of this call's result to the 16-bit type IS the 16-bit call's result, bit for bit, for beta == 0 and, when the old `out` is representable in 16 bits,
 *     for beta != 0 (every leaf rounds to f32 first).
 * Which kernels: the plan is the 16-bit planner's for the same query (shape, leading dimensions, matrix strides and base addresses as they are, each in its own
 * operand's elements) with the continuous tile walk and the panel form off (wg_debug_gemm_out32_query). Every other leaf is taken: the few-column kernel, 128 x 128
 * with and without a K cut, 256 x 128, the 256 x 256 per-tile kernel (static map, tile queues, calibrated shares, split-K, cut-up tail), the padded call, the
 * generic kernel; the WG_TUNE_F16_* knobs apply as they do to bf16. Every leaf stores f32 directly at any 4-byte-aligned address: an `out` view at an odd offset,
 * with an odd leading dimension and an odd gap between matrices runs where it lies. The few-column leaf stores directly too (its one-split form writes the four
 * floats of a lane; with a K cut it writes the usual f32 slabs and the f32 slab reduce finishes). The call never takes the Gemv kernels: the "1 .. 7 columns run as
 * a Gemv" shortcut of wg_gemm_ex has no 16-bit x 16-bit -> f32 kernel to go to, and the 16-bit tile kernels take any N as it is. M or K not a multiple of 4:
 * staged like wg_gemm_ex, the output's copy in f32.
 *   ALIASED       : `out` shares a byte with `m1` or with `m2` -- on addresses, in 2-byte units as wg_gemv_mixed does, so `out` and `m1` may live in one buffer:
 *                   touching is legal, one shared byte is refused. `m1` and `m2` may overlap each other.
 * Not included: the row-major surface (wg_gemm_rm), the sharded / panel calls (wg_gemm_sharded*), the continuous walk.
 * wg_debug_take_path: the element prefix is "f16o32." / "bf16o32."; the dtype-free tags ("splitk.reduce/ns=", "stage..>") are unchanged.
 */
int wg_gemm_out32(wg_ctx *ctx, wg_gemm_variant variant, wg_dtype in_dtype, float alpha, float beta,
                  wg_buf *out, wg_view_shape out_shape,
                  const wg_buf *m1, wg_view_shape m1_shape,
                  const wg_buf *m2, wg_view_shape m2_shape);

/*
 * Extension: Gemm on 8-bit weights with group scales and 16-bit columns -- wg_gemv_q8's matrix, in its layout, against N columns of f16 / bf16 activations on the
 * matrix cores (batched decode, speculative decoding, short prefill: the counterpart of wg_gemv_q8 as wg_gemm_out32 is of wg_gemv_mixed). out = W^T x with
 * W[r, c, z] = scales[r / G, c, z] * (float)m[r, c, z], G = group_rows: `m` holds int8_t, k x outputs x mats, column-major (k contiguous; all 256 values are legal);
 * `scales` holds f32, ceil(k / G) x outputs x mats; `x` holds x_dtype elements (WG_F16 or WG_BF16), k x N x mats; `out` holds f32, outputs x N x mats. Groups run
 * along the rows of `m`, the contraction. The same `m` and `scales` buffers serve wg_gemv_q8. No alpha, no beta: `out` is overwritten. Every view shape counts
 * elements of its own operand's type; the bounds checks use 1 / 4 / 2 / 4 bytes per element of m / scales / x / out. wg_dtype has no 8-bit value and gets none.
 *   variant       : WG_GEMM_TR and WG_GEMM_TR_FAST are the product above (_FAST is the same call). WG_GEMM and WG_GEMM_FAST would be out = W x, with the groups along the
 *                   OUTPUT rows and one scale per k index and row group: there the scale cannot leave the contraction, so a 16-bit MFMA would have to round s * q or
 *                   s * x to 16 bits, and this call narrows nothing. They return WG_ERR_UNSUPPORTED ("... wg_gemv_q8 computes out = W v ...").
 *   x_dtype       : WG_F16 or WG_BF16. WG_F32 is WG_ERR_UNSUPPORTED (f32 activations stay with wg_gemv_q8; the message names it); anything else WG_ERR_INVALID_ARG.
 *   group_rows    : as wg_gemv_q8 -- a positive multiple of 16, or any positive value >= k (one scale per output). Anything else is WG_ERR_INVALID_ARG.
 *   DIM_MISMATCH  : the Gemm check with its message (m.rows == x.rows, out.rows == m.cols, out.cols == x.cols, equal mats); then `scales` of another shape than
 *                   the one above ("Gemm: dimension mismatch. (m [..], group_rows G, scales [..], expected [..])").
 * Everything else is wg_gemm_out32's / wg_gemv_q8's contract, in their order, with their status codes: the NULL context ("Gemm: ctx is NULL"), NULL buffers, the
 * unknown variant, zero-sized buffers / views skipped with WG_OK, views that exceed their buffer, WG_ERR_WORKSPACE when the partials of a cut contraction would
 * have to grow the context's workspace inside a recording; mats * column passes > 65535 is WG_ERR_UNSUPPORTED.
 * Arithmetic:
 *   - int8 -> f16 / bf16 is exact for all 256 values; `x` is read as the 16-bit value it is; every product is exact in f32 inside the MFMA;
 *   - the scale enters per GROUP (the streaming kernel): d = the MFMA chain over the group's 32-row steps, started from zero, then acc = fmaf(scale, d, acc) in f32
 *     on the vector ALU, groups ascending. A step never straddles a group. The unscaled d must be finite for a finite result. On any other view (the
 *     element-by-element kernel): w = scale * q, acc = fmaf(w, (float)x, acc). Each of the k terms takes at most two f32 roundings either way;
 *   - the f32 accumulator is stored as it is. Nothing is flushed: subnormal scales and subnormal results are kept;
 *   - Inf and NaN behave as in the f32 product of the dequantised matrix with `x` (a zero weight or a zero scale against an Inf gives NaN) and reach exactly the
 *     outputs whose sums contain them; load slots past the end of k and columns / outputs past the edge of a tile contribute nothing and are not stored;
 *   - deterministic: no atomics; a cut contraction writes f32 partials that one pass adds in a fixed order -- two calls give identical bits.
 * Which kernels (gemm_q8_plan.hip, wg_debug_gemm_q8_plan): the streaming kernel takes views where k % 32 == 0 (a k that is only a multiple of 16 is NOT taken:
 * there is no zero-filled half step), group_rows % 32 == 0 or group_rows >= k, and the first element, leading dimension and matrix stride of `m` and of `x` are
 * multiples of 16 bytes; `out` is stored one float at a time (128 contiguous bytes per wave-instruction) and may be any 4-byte-aligned view. A wave owns 32 outputs
 * and 32 or 64 columns; N past 64 re-reads the weights once per pass of 64 columns (the call is for about 9 .. 128 columns). Every other view runs where it lies on
 * the element-by-element kernel -- correct, not fast, no padded copies.
 *   ALIASED       : `out` shares a byte with the part of `m`, of `scales` or of `x` the call addresses -- on addresses, `m` in 1-byte and `x` in 2-byte units, so
 *                   they may live in one buffer: touching is legal, one shared byte is refused. The read operands may overlap each other.
 * Not included: out = W x, alpha / beta, f32 activations, the row-major and sharded surfaces. int8 activations are wg_gemm_q8a8's.
 * wg_debug_take_path: tags begin "gemm_q8/": "gemm_q8/mfma,f16,nt=4,ns=8" (x's element, 16-column tiles per wave, splits), "gemm_q8/combine,ns=8", "gemm_q8/any".
 */
int wg_gemm_q8(wg_ctx *ctx, wg_gemm_variant variant, uint32_t group_rows, wg_dtype x_dtype,
               wg_buf *out, wg_view_shape out_shape,             /* f32: outputs x N x mats */
               const wg_buf *m, wg_view_shape m_shape,           /* int8_t: k x outputs x mats, column-major */
               const wg_buf *scales, wg_view_shape scales_shape, /* f32: ceil(k / group_rows) x outputs x mats */
               const wg_buf *x, wg_view_shape x_shape);          /* x_dtype (WG_F16 or WG_BF16): k x N x mats */

/*
 * Extension: Gemm on packed 4-bit weights with group scales and 16-bit columns -- wg_gemv_q4's matrix and scales, byte for byte, against N columns of f16 / bf16
 * activations on the matrix cores (the counterpart of wg_gemv_q4 as wg_gemm_q8 is of wg_gemv_q8). out = W^T x. `m` holds packed BYTES, k / 2 x outputs x mats,
 * column-major: byte j of a column holds logical row 2 j in its LOW nibble and row 2 j + 1 in its HIGH nibble; a nibble n in 0 .. 15 stands for q = n - 8, all 16
 * values are legal; W[r, c, z] = scales[r / G, c, z] * (float)q[r, c, z], G = group_rows. m_shape counts BYTES (rows, leading dimension, offset, matrix stride) and
 * k = 2 * m.rows. `scales` holds f32, ceil(k / G) x outputs x mats; `x` holds x_dtype elements (WG_F16 or WG_BF16), k x N x mats; `out` holds f32, outputs x N x mats.
 * The same `m` and `scales` buffers serve wg_gemv_q4. No alpha, no beta: `out` is overwritten. The bounds checks use 1 / 4 / 2 / 4 bytes per element of m / scales /
 * x / out. wg_dtype has no 4-bit value and gets none.
 *   variant       : WG_GEMM_TR and WG_GEMM_TR_FAST are the product above (_FAST is the same call). WG_GEMM and WG_GEMM_FAST return WG_ERR_UNSUPPORTED ("... wg_gemv_q8
 *                   computes out = W v ..."), right behind the checks of the context, the buffers, x_dtype and the variant's range and BEFORE any dimension,
 *                   group_rows or size is looked at, as wg_gemm_q8 and wg_gemv_q4 do: a mismatched or zero-sized call with these variants is UNSUPPORTED too.
 *   x_dtype       : WG_F16 or WG_BF16. WG_F32 is WG_ERR_UNSUPPORTED (f32 vectors stay with wg_gemv_q4; the message names it); anything else WG_ERR_INVALID_ARG.
 *   group_rows    : wg_gemv_q4's rule -- a positive multiple of 32, or any positive value >= k (one scale per output). Anything else is WG_ERR_INVALID_ARG.
 *   DIM_MISMATCH  : x.rows != 2 * m.rows, out.rows != m.cols, out.cols != x.cols or unequal mats ("Gemm: dimension mismatch. (out [..], m1 [..]^T packed: k K,
 *                   m2 [..])"); then `scales` of another shape than the one above ("Gemm: dimension mismatch. (m [..] packed: k K, group_rows G, scales [..],
 *                   expected [..])").
 * Everything else is wg_gemm_q8's contract, in its order, with its status codes: the NULL context ("Gemm: ctx is NULL"), NULL buffers, the unknown variant,
 * zero-sized buffers / views skipped with WG_OK, views that exceed their buffer, WG_ERR_WORKSPACE when the partials of a cut contraction would have to grow the
 * context's workspace inside a recording; mats * column passes > 65535 is WG_ERR_UNSUPPORTED.
 * Arithmetic:
 *   - q = n - 8 is formed exactly IN THE 16-BIT TYPE before any product (f16: (1024 + n) - 1032 and fma(1024 + 16 n, 1/16, -72), both exact; bf16: n as f32, minus
 *     8, its high half). The -8 is never folded into a correction of the sum: a nibble of 8 is a true zero -- against a finite x it adds exactly nothing, against
 *     Inf it gives NaN. `x` is read as the 16-bit value it is; every product is exact in f32 inside the MFMA;
 *   - the scale enters per GROUP (the streaming kernel): d = the MFMA chain over the group's 32-row steps, started from zero, then acc = fmaf(scale, d, acc) in f32
 *     on the vector ALU, groups ascending. A chain never holds rows of two groups (groups of 32 included). The unscaled d must be finite for a finite result. On
 *     any other view (the element-by-element kernel): w = scale * q, acc = fmaf(w, (float)x, acc), even row first. Each of the k terms takes at most two f32
 *     roundings either way;
 *   - the f32 accumulator is stored as it is. Nothing is narrowed or flushed: subnormal scales and subnormal results are kept;
 *   - Inf and NaN behave as in the f32 product of the dequantised matrix with `x` and reach exactly the outputs whose sums contain them; load slots past the end
 *     of k and columns / outputs past the edge of a tile contribute nothing and are not stored;
 *   - deterministic: no atomics; a cut contraction writes f32 partials that one pass adds in a fixed order -- two calls give identical bits.
 * Which kernels (gemm_q4_plan.hip, wg_debug_gemm_q4_plan): the streaming kernel takes views where k % 32 == 0 -- the step is 32 logical rows; a lane's 16-byte load
 * covers half of a 64-row double step and the halves of a wave exchange dwords, but a last double step of 32 rows is taken, so the condition is NOT k % 64 == 0 --,
 * group_rows % 32 == 0 or group_rows >= k, and the first byte, leading dimension and matrix stride of `m` and the first element, leading dimension and matrix
 * stride of `x` are multiples of 16 bytes; `scales` and `out` are reached one float at a time and may be any 4-byte-aligned view. A wave owns 32 outputs and 32 or
 * 64 columns; N past 64 re-reads the weights once per pass of 64 columns. Every cut boundary is a multiple of 32 and, where group_rows < k, of group_rows. Every
 * other view runs where it lies on the element-by-element kernel (a wave per output, a byte -- two weights -- per lane and step): correct, not fast, no padded copies.
 *   ALIASED       : `out` shares a byte with the part of `m`, of `scales` or of `x` the call addresses -- on addresses, `m` in 1-byte and `x` in 2-byte units, so
 *                   they may live in one buffer: touching is legal, one shared byte is refused. The read operands may overlap each other.
 * Not included: out = W x, alpha / beta, zero points, f32 or int8 activations (int8 against 8-bit weights: wg_gemm_q8a8), the row-major and sharded surfaces.
 * wg_debug_take_path: tags begin "gemm_q4/": "gemm_q4/mfma,f16,nt=2,ns=1" (x's element, 16-column tiles per wave, splits), "gemm_q4/combine,ns=8", "gemm_q4/any".
 */
int wg_gemm_q4(wg_ctx *ctx, wg_gemm_variant variant, uint32_t group_rows, wg_dtype x_dtype,
               wg_buf *out, wg_view_shape out_shape,             /* f32: outputs x N x mats */
               const wg_buf *m, wg_view_shape m_shape,           /* packed bytes: k / 2 x outputs x mats, column-major */
               const wg_buf *scales, wg_view_shape scales_shape, /* f32: ceil(k / group_rows) x outputs x mats */
               const wg_buf *x, wg_view_shape x_shape);          /* x_dtype (WG_F16 or WG_BF16): k x N x mats */

/*
 * Extension: Gemm on 8-bit weights AND 8-bit activations, both with f32 group scales (W8A8: per-channel weights x per-token activations, or Q8_0 x Q8_1-style groups
 * on both sides), on the i8 matrix cores. out = W^T X with W[r, c, z] = scales[r / G, c, z] * m[r, c, z] and X[r, j, z] = x_scales[r / Gx, j, z] * x[r, j, z],
 * G = group_rows, Gx = x_group_rows. `m` and `scales` are wg_gemv_q8's and wg_gemm_q8's buffers, byte for byte; `x` holds int8_t, k x N x mats, column-major;
 * `x_scales` f32, ceil(k / Gx) x N x mats; `out` f32, outputs x N x mats. All 256 int8 values are legal on both sides. No alpha, no beta: `out` is overwritten. The
 * bounds checks use 1 / 4 / 1 / 4 / 4 bytes per element of m / scales / x / x_scales / out. wg_quantize_q8 below makes `x` and `x_scales` on the device.
 *   variant       : WG_GEMM_TR and WG_GEMM_TR_FAST are the product above (_FAST is the same call). WG_GEMM and WG_GEMM_FAST return WG_ERR_UNSUPPORTED ("... wg_gemv_q8
 *                   computes out = W v ..."), right behind the checks of the context, the buffers and the variant's range and BEFORE any dimension, group size or
 *                   size is looked at, as wg_gemm_q8 does.
 *   group sizes   : group_rows and x_group_rows are each a positive multiple of 16, or any positive value >= k (one scale per output / per column). Where both are
 *                   below k one must divide the other. Anything else is WG_ERR_INVALID_ARG.
 *   DIM_MISMATCH  : the Gemm check with wg_gemm_q8's message; then `scales` of another shape than the one above ("Gemm: dimension mismatch. (m [..], group_rows G,
 *                   scales [..], expected [..])"); then `x_scales` ("Gemm: dimension mismatch. (x [..], x_group_rows Gx, x_scales [..], expected [..])").
 * Everything else is wg_gemm_q8's contract, in its order, with its status codes: the NULL context ("Gemm: ctx is NULL"), NULL buffers, the unknown variant,
 * zero-sized buffers / views skipped with WG_OK, views that exceed their buffer, WG_ERR_WORKSPACE when the partials of a cut contraction would have to grow the
 * context's workspace inside a recording; mats * column passes > 65535 is WG_ERR_UNSUPPORTED.
 * Arithmetic -- ONE definition for every kernel; the bits of an uncut call do not depend on which kernel ran:
 *   - the contraction is divided into CHAINS: a chain ends at every boundary of a weight group and of an activation group and, inside the finer of the two groups,
 *     every 1024 rows counted from that group's start;
 *   - d = the chain's integer sum of m * x in int32, exact: |d| <= 1024 * 128 * 128 = 2^24, so (float)d is exact too (without the cap an int32 chain overflows
 *     from 2^17 rows on and (float)d rounds from 1025 rows on: the cap is part of the contract);
 *   - u = x_scale * (float)d, one f32 multiply; acc = fmaf(w_scale, u, acc), chains ascending (a tiny weight scale never enters an intermediate product);
 *   - the f32 accumulator is stored as it is. Nothing is narrowed or flushed: subnormal scales and results are kept;
 *   - non-finite scales behave as these two f32 operations say (0 * Inf is NaN) and reach exactly the outputs whose chains hold them;
 *   - deterministic: no atomics; a cut contraction writes f32 partials [z][split][n][outputs] that one pass adds in gemm_q8's fixed order (wave w adds splits w,
 *     w + 4, ... ascending, then the four are added ascending) -- two calls give identical bits. A cut changes the bits (its partial sums start from zero).
 * Which kernels (gemm_q8a8_plan.hip, wg_debug_gemm_q8a8_plan): the streaming kernel takes views where k % 32 == 0, each group size % 32 == 0 or >= k, and the first
 * element, leading dimension and matrix stride of `m` and of `x` are multiples of 16 bytes; the scales and `out` are reached one float at a time and may be any
 * 4-byte-aligned view. Both operands go into v_mfma_i32_32x32x32_i8 exactly as loaded: no conversion. A wave owns 32 outputs and 32 or 64 columns; N past 64 re-reads
 * the weights once per pass of 64 columns. Every cut boundary is a chain boundary. Every other view runs where it lies on the element-by-element kernel: the same
 * chains, the same two f32 operations, no padded copies.
 *   ALIASED       : `out` shares a byte with the part of `m`, `scales`, `x` or `x_scales` the call addresses -- on addresses, `m` and `x` in 1-byte units: touching is
 *                   legal, one shared byte is refused. The read operands may overlap each other.
 * Not included: out = W x, alpha / beta, 4-bit weights against int8 activations, zero points, the row-major and sharded surfaces.
 * wg_debug_take_path: tags begin "gemm_q8a8/": "gemm_q8a8/mfma,nt=2,ns=1" (16-column tiles per wave, splits), "gemm_q8a8/combine,ns=8", "gemm_q8a8/any".
 */
int wg_gemm_q8a8(wg_ctx *ctx, wg_gemm_variant variant, uint32_t group_rows, uint32_t x_group_rows,
                 wg_buf *out, wg_view_shape out_shape,                  /* f32: outputs x N x mats */
                 const wg_buf *m, wg_view_shape m_shape,                /* int8_t: k x outputs x mats, column-major */
                 const wg_buf *scales, wg_view_shape scales_shape,      /* f32: ceil(k / group_rows) x outputs x mats */
                 const wg_buf *x, wg_view_shape x_shape,                /* int8_t: k x N x mats, column-major */
                 const wg_buf *x_scales, wg_view_shape x_scales_shape); /* f32: ceil(k / x_group_rows) x N x mats */

/*
 * Extension: the device-side quantiser of the q8 family -- activations (k x N) and weights (k x outputs) alike. The rule is the Python helper quantize_q8's on the
 * source widened exactly to f32: per group of group_rows consecutive rows of a column (a partial last group) s = fl32(max|x| / 127) and
 * q = clip(rint(fl32(x / s)), -127, 127) -- a true IEEE division per element (not a multiply by a reciprocal: the two differ at ties), rounding ties to even, the
 * clamp before the integer conversion; -128 is never produced. s == 0 (an all-zero group, or one whose max / 127 rounds to zero) gives q = 0. A group whose
 * max|x| is not finite (it holds a NaN or an Inf) gets s = NaN and q = 0 throughout.
 * `q` holds int8_t, rows x cols x mats; `scales` f32, ceil(rows / group_rows) x cols x mats; `src` holds src_dtype elements (WG_F32, WG_F16, WG_BF16) in q's shape.
 *   group_rows    : a positive multiple of 16, or any positive value >= rows (one scale per column). Anything else is WG_ERR_INVALID_ARG.
 *   DIM_MISMATCH  : "Quantize: dimension mismatch. (q [..], src [..])", then "Quantize: dimension mismatch. (q [..], group_rows G, scales [..], expected [..])".
 * NULL context / buffers and an unknown src_dtype are WG_ERR_INVALID_ARG; zero-sized buffers / views are skipped with WG_OK; a view that exceeds its buffer is
 * WG_ERR_OUT_OF_BOUNDS (1 / 4 / src bytes per element of q / scales / src); more than 2^31 - 1 workgroups or 65535 matrices is WG_ERR_UNSUPPORTED.
 *   ALIASED       : `q` or `scales` shares a byte with the addressed part of `src`, or with each other (on addresses, in 1-byte units).
 * It needs no workspace and works inside a recording. Deterministic.
 * Which kernels (quantize_q8.hip, wg_debug_quantize_q8_plan): group_rows in 32, 64, .. 1024 (a power of two), rows % 16 == 0 and first element, leading dimension
 * and matrix stride of `q` and `src` multiples of 16 bytes: a lane per 16 rows, 16-byte accesses, the group's max by cross-lane exchange. Everything else, one scale
 * per column included: a wave (groups up to 1024 rows) or a workgroup per (group, column), two sweeps, where it lies.
 * wg_debug_take_path: "quantize_q8/vec,f16", "quantize_q8/any,bf16" (the source's element).
 */
int wg_quantize_q8(wg_ctx *ctx, wg_dtype src_dtype, uint32_t group_rows,
                   wg_buf *q, wg_view_shape q_shape,            /* int8_t: rows x cols x mats */
                   wg_buf *scales, wg_view_shape scales_shape,  /* f32: ceil(rows / group_rows) x cols x mats */
                   const wg_buf *src, wg_view_shape src_shape); /* src_dtype (WG_F32, WG_F16, WG_BF16): rows x cols x mats */

/*
 * ROW_MAJOR operator surface. Replaces composing the reference's shaders with
 * `row_major_shader_defs()` (wgebra linalg/shape.rs:11-15): every matrix view of the call is ROW-major,
 * index = t*stride_mat + offset + i*stride + j (shape.wgsl:49-52), `stride` = elements between consecutive ROWS;
 * the vec4 precondition becomes cols, stride, stride_mat, offset % 4 == 0 (shape.wgsl:54-56). Same dimension checks
 * and messages as wg_gemm / wg_gemv. A row-major view is the column-major view of the transpose, so WG_GEMM runs the
 * column-major kernel with the operands swapped (no copy); WG_GEMM_TR needs m1 transposed in memory first (one HBM-bound
 * pass into a context-owned scratch buffer). wg_gemv_rm with several right-hand-side columns (ncols % 4 == 0, the row-major
 * vec4 precondition) runs as the row-major Gemm / GemmTr it is.
 * ALIASED: as wg_gemm / wg_gemv (the aliasing rule; a row-major view covers the same elements as its column-major twin), whichever kernels the call would take --
 * the GemmTr that first copies m1 into scratch refuses an `out` that overlaps `m1` like the one that reads m1 where it lies.
 */
int wg_gemm_rm(wg_ctx *ctx, wg_gemm_variant variant, wg_dtype dtype,
               wg_buf *out, wg_view_shape out_shape,
               const wg_buf *m1, wg_view_shape m1_shape,
               const wg_buf *m2, wg_view_shape m2_shape);
int wg_gemv_rm(wg_ctx *ctx, wg_gemv_variant variant, wg_dtype dtype,
               wg_buf *out, wg_view_shape out_shape,
               const wg_buf *m, wg_view_shape m_shape,
               const wg_buf *v, wg_view_shape v_shape);

/*
 * Reduce::dispatch (wgebra reduce.rs:100-113): result[0] = reduce(op, value[offset .. offset+size[0])).
 * `result` is the GpuScalar's buffer (>= 4 bytes). The summation ORDER is the reference's (128 strided lanes,
 * then the 64..1 tree; reduce.wgsl:68-87), so Min/Max/Sum/Prod are bit-identical to it; n == 0 gives the init
 * value (0, 1, +3.4e38, -3.4e38).
 * dtype WG_F16 (extension): `value` and `result` are f16; elements are converted to f32 (exact), folded in the same order in f32,
 * and the result is rounded once (RNE) to f16. (wg_reduce_batched and wg_reduce_fast likewise.) WG_BF16 (extension): likewise on bfloat16 (widening is exact).
 * ALIASED: the result element (result[0]) lies inside value[offset .. offset+size[0]) (the aliasing rule). A result directly before or behind the vector is legal.
 */
int wg_reduce(wg_ctx *ctx, wg_reduce_op op, wg_dtype dtype,
              const wg_buf *value, wg_view_shape value_shape, wg_buf *result);

/*
 * Extension: result[0] = reduce(op, op(m) * v) in one call (e.g. SqNorm for |m v|^2, Max for the largest entry).
 * Launch-bound sizes (Gemv, rows * cols <= 4 Mi, rows >= 128) run as ONE kernel: the last workgroup to finish folds the product
 * vector in the reference order (reduce.wgsl:68-87); everything else is Gemv into a context-owned scratch vector, then Reduce, on the
 * same stream. Either way bit-identical to wg_gemv followed by wg_reduce; `m` is one matrix, `v` one vector.
 * ALIASED: result[0] lies inside `m` or inside `v` (the aliasing rule). The product vector is context-owned scratch and aliases nothing of the caller's.
 */
int wg_gemv_reduce(wg_ctx *ctx, wg_gemv_variant variant, wg_reduce_op op, wg_dtype dtype, wg_buf *result,
                   const wg_buf *m, wg_view_shape m_shape, const wg_buf *v, wg_view_shape v_shape);

/*
 * Extension: two-pass, multi-workgroup reduce of ONE long vector at HBM speed. Same arguments and
 * checks as wg_reduce, but NOT the reference's summation order (which serialises a vector onto one workgroup): Min/Max
 * are bit-identical to wg_reduce, Sum/Prod/SqNorm are re-associated -- deterministic (fixed chunking and tree, no
 * atomics) and within n * 2^-24 * sum|x| (sum x^2 for SqNorm) of the reference order. ALIASED: as wg_reduce.
 */
int wg_reduce_fast(wg_ctx *ctx, wg_reduce_op op, wg_dtype dtype,
                   const wg_buf *value, wg_view_shape value_shape, wg_buf *result);

/*
 * Extension (BASELINE config 4): one launch for many vectors. Column c of matrix t of the
 * column-major view is reduced exactly as wg_reduce would reduce the vector view at
 * offset + c*stride + t*stride_mat; results[c + t*size[1]] (one element of `dtype` each).
 * ALIASED: one of the size[1] * size[2] result elements lies inside the `values` view (the aliasing rule).
 */
int wg_reduce_batched(wg_ctx *ctx, wg_reduce_op op, wg_dtype dtype,
                      const wg_buf *values, wg_view_shape values_shape, wg_buf *results);

/*
 * OpAssign::dispatch (wgebra op_assign.rs:71-95): a[i] = a[i] (op) b[i], i < a.size[0]; WG_OP_COPY: a[i] = b[i].
 * Scalar indexing offset+i (shape.wgsl:36-38). DIM_MISMATCH: a.size[0] != b.size[0] (op_assign.rs:82-86).
 * IEEE-correct + - * / : bit-identical to the reference's CPU check.
 * ALIASED: `a` and `b` overlap partly (the aliasing rule). Extension: `b` may be the IDENTICAL view -- same address, same length: every lane loads its a[i] and
 * b[i] before it stores a[i], so the result is x (op) x to the bit (a += a doubles, a /= a gives 1, and NaN where IEEE says so: 0 / 0, Inf / Inf).
 */
int wg_op_assign(wg_ctx *ctx, wg_op_assign_variant op, wg_dtype dtype,
                 wg_buf *a, wg_view_shape a_shape, const wg_buf *b, wg_view_shape b_shape);

/*
 * Extension (the north-star's "Axpy" -- the reference has no such operator, only OpAssign):
 * y[i] = fma(alpha, x[i], y[i]), i < y.size[0], one rounding per element. alpha = +1 / -1 reproduce WG_OP_ADD / WG_OP_SUB
 * (as `y += x` / `y -= x`) bit for bit. Same indexing, errors and skips as wg_op_assign. f16 and bf16: computed in f32, rounded once.
 * ALIASED: as wg_op_assign -- a partial overlap of `y` and `x` is refused, the identical view is allowed (y[i] = fma(alpha, y[i], y[i])).
 */
int wg_axpy(wg_ctx *ctx, float alpha, wg_dtype dtype, wg_buf *y, wg_view_shape y_shape, const wg_buf *x, wg_view_shape x_shape);

/*
 * Extension (strided / offset views): dst view = src view where the source has elements, 0 where it has none
 * (dst.size[0] x dst.size[1] per matrix; rows / columns of `src` beyond dst's are dropped). Any offset, stride and length on either side --
 * 16-byte accesses with a byte shift whatever the alignment (transpose.hip). It is the pass wg_gemm* / wg_gemv* run for operands that are
 * not vec4-aligned; a caller that multiplies the same odd view many times makes the aligned copy ONCE with this and passes that instead.
 * DIM_MISMATCH: dst.size[2] != src.size[2]. Zero-sized views: skipped. ALIASED: `dst` shares a byte with `src` (the aliasing rule; no exception for identical
 * views: a copy onto itself is refused like a copy shifted by one row).
 */
int wg_copy_view(wg_ctx *ctx, wg_dtype dtype, wg_buf *dst, wg_view_shape dst_shape, const wg_buf *src, wg_view_shape src_shape);

/* ------------------------------------------------------------------------------------------------ */
/* multi-GPU: the M-sharded Gemm of the north star. The reference has one wgpu::Device + Queue       */
/* (wgcore gpu.rs:7-12) and nothing to replace here; what is kept is its tensor model: every rank's   */
/* operands and the gathered result are plain column-major tensors addressed by ViewShape, and each   */
/* rank's local product is Gemm::dispatch_generic (gemm.rs:65-127) on views of them.                  */
/* ------------------------------------------------------------------------------------------------ */
typedef struct wg_comm wg_comm; /* one rank of a group of contexts (one context = one GPU); not thread-safe, like its context */
#define WG_COMM_ID_BYTES 128   /* == sizeof(ncclUniqueId) */
#define WG_IPC_HANDLE_BYTES 96
typedef enum wg_gather_mode {
    WG_GATHER_RCCL = 0,      /* per N-panel: Gemm into a staging cube [M/P, np, P], in-place ncclAllGather (RCCL over xGMI) on the
                                communicator's stream beside the next panel's Gemm, then an HBM-bound relayout into columns of C */
    /* 1 was WG_GATHER_PEER_COPY (Gemm straight into C + hsa_amd_memory_async_copy_rect pushes by a helper thread): removed in ABI 3 -- one
       rect-capable SDMA queue per direction made it a 2-rank engine at best, and it could hang two processes sharing a GPU at 32768^3 */
    WG_GATHER_NONE = 2,      /* this rank's rows of C only */
    WG_GATHER_PEER_STAGED = 3 /* per N-panel: Gemm into slot g of this rank's staging cube, one CONTIGUOUS copy per peer (the runtime's
                                peer-to-peer path: that link's own SDMA engine, no compute units) into the same slot of the peer's cube + a
                                sequence-number flag; the receiver's stream waits on the flags (one-wave kernel) and relayouts the panel into
                                C. Stream-ordered end to end, no barrier: the cubes are double-buffered by step parity. Needs
                                wg_comm_stage_reserve + wg_comm_set_peer_stages. The copy-engine exchange for any P.
                                The HIP runtime folds a process's streams onto 4 hardware queues unless GPU_MAX_HW_QUEUES says otherwise: give
                                a rank's process >= 3 + P of them, or its copies queue up behind its Gemms instead of running beside them
                                (correct either way; two ranks driven from ONE thread on one device need it for progress) */
} wg_gather_mode;

/* ncclGetUniqueId: call on one rank, ship the WG_COMM_ID_BYTES bytes to the others out of band (env, file, MPI, a torch store). */
int wg_comm_unique_id(void *id);
/* Rank `rank` of `nranks`, bound to `ctx` (its device, its stream). id != NULL: ncclCommInitRank (collective: every rank must call).
 * id == NULL: no collective library -- staged peer copies only, the caller brings its own barrier. librccl is bound at run time;
 * the library itself links only the HIP runtime. */
int wg_comm_create(wg_ctx *ctx, int nranks, int rank, const void *id, wg_comm **out);
int wg_comm_destroy(wg_comm *comm);
int wg_comm_rank(const wg_comm *comm);
int wg_comm_size(const wg_comm *comm);
int wg_comm_has_collectives(const wg_comm *comm);
int wg_comm_reported_size(const wg_comm *comm, int *count); /* ncclCommCount: the rank count the collective library itself reports (0 without one) */
uint64_t wg_comm_bytes_sent(const wg_comm *comm);     /* payload bytes this rank contributed / pushed so far */
/* In-place all-gather of elements [first, first + nranks*per_rank) of `buf` (rank r owns [first + r*per_rank, +per_rank)) on the
 * communicator's stream, ordered after the work already enqueued on the context; the context does not wait (wg_comm_join). */
int wg_all_gather(wg_comm *comm, wg_dtype dtype, wg_buf *buf, uint64_t first_elem, uint64_t elems_per_rank);
int wg_comm_join(wg_comm *comm);    /* the context's stream waits for the collectives in flight (and completes a deferred last panel) */
/* Pipelined steps (WG_GATHER_PEER_STAGED, and WG_GATHER_RCCL in its one-launch form): with on != 0 a wg_gemm_sharded call leaves the wait + relayout of its LAST panel -- the one
 * exchange nothing of its own call can hide -- to the next call on the communicator, which runs it right after enqueueing its first Gemm
 * (wg_comm_join / _flush / _barrier / a call in another mode complete it too). `out` is then complete in stream order only after that. */
/* One launch per step: an f16 wg_gemm_sharded of at least one round of 256 x 256 tiles (WG_GATHER_RCCL, WG_GATHER_PEER_STAGED, panels of whole
 * tiles) can run the rank's product as ONE kernel over all N-panels; the kernel writes each panel through to memory, its waves count
 * themselves into a per-panel word, the exchange of a panel waits for the full count (hipStreamWaitValue32) and the relayouts follow the
 * kernel. Bit for bit the result of the panel-by-panel launches (whenever those are not split along K). on = 1 / 0 force it / the panel
 * launches, on < 0 (default) decides by engine: RCCL on -- the scheduler-driven launch does not care how many CUs its stream has, so
 * RCCL's copy kernels need only 8 of them instead of 32 --, staged off (measured 1-2 % slower than 16 synchronised one-round launches). */
int wg_comm_set_one_launch(wg_comm *comm, int on);
/* Diagnostics: with on != 0 every later wg_gemm_sharded call stamps the context's stream right before and right after each "wait for panel p's
 * exchange" (a pair of timing events; a few microseconds of host time per panel -- leave it off in timed regions). wg_comm_wait_times synchronises
 * the context, returns (panel, milliseconds the compute stream stood still) for up to `capacity` waits since the last call, oldest first, and
 * starts over. An exchange that hid under the Gemms reads ~0; a slow link shows up as the waits of a step's FIRST relayouts, a slow rank as waits
 * on every panel of its peers, the un-hidden tail as the last panel's wait. */
int wg_comm_set_wait_timing(wg_comm *comm, int on);
int wg_comm_wait_times(wg_comm *comm, uint32_t *panels, float *ms, uint32_t capacity, uint32_t *count);
int wg_comm_set_pipelined(wg_comm *comm, int on); /* (a step with ONE panel always completes in its call: deferring it would let a rank run two steps ahead of a peer) */
int wg_comm_flush(wg_comm *comm);   /* host-blocking: every peer copy this rank issued has landed */
int wg_comm_barrier(wg_comm *comm); /* flush + a one-element all-reduce joined into the context: all ranks' earlier exchanges are complete */
/* One process per GPU: export a device buffer / map a peer's (hipIpcGetMemHandle / hipIpcOpenMemHandle; needs the dmabuf IPC mode,
 * HSA_ENABLE_IPC_MODE_LEGACY=0, on this platform). The mapped buffer is released by wg_buf_destroy. */
int wg_buf_ipc_export(const wg_buf *buf, void *handle /* WG_IPC_HANDLE_BYTES */);
int wg_buf_ipc_open(wg_ctx *ctx, const void *handle, wg_buf **out);
/* WG_GATHER_PEER_STAGED: make the communicator's staging cubes (>= 2 * sizeof(T) * M * N bytes: two steps in flight) and its flag array
 * exist and return them (owned by the communicator) so that the caller can export them (wg_buf_ipc_export) to the peers; then register
 * every peer's pair as addressable from here (wg_buf_ipc_open, or the buffers themselves when the ranks share a process). Growing the
 * cubes invalidates the registration on every rank. EVERY RANK MUST RESERVE THE SAME SIZE: the two step-parity halves sit at offsets 0
 * and bytes / 2 whatever the shape of a step (wg_comm_set_peer_stages checks it), which is what lets M / N / panel_cols change between
 * steps without a barrier. A receiver waits WG_COMM_TIMEOUT_MS (environment, read when the communicator is created; default 30000) for
 * a peer's slot; after that the panel's columns of `out` are filled with NaN bit patterns and the error is returned by the next
 * wg_ctx_sync / wg_buf_read on the context, wg_comm_flush / _join / _barrier, or wg_gemm_sharded call -- never a hung queue, never stale data. */
int wg_comm_stage_reserve(wg_comm *comm, size_t bytes, wg_buf **stage, wg_buf **flags);
int wg_comm_set_peer_stages(wg_comm *comm, wg_buf *const *peer_stage, wg_buf *const *peer_flags);
/* Relayout of a gathered GpuCube [M/P, np, P] (dense) into the (M x np) column-major view `out`: out[g*M/P + i, j] = cube[i, j, g].
 * HBM-bound: 2 * sizeof(T) * M * np bytes. (What WG_GATHER_RCCL runs per panel; exported for callers that gather themselves.) */
int wg_cube_to_matrix(wg_ctx *ctx, wg_dtype dtype, const wg_buf *cube, wg_view_shape cube_shape, wg_buf *out, wg_view_shape out_shape);
/*
 * out (M x N, one matrix, on EVERY rank) = op(A) * B with A sharded on M: `a_rows` is this rank's row block of op(A)
 * (M/P x K; WG_GEMM_TR*: stored K x M/P), `b` (K x N) is replicated. N is cut into panels of `panel_cols` columns (0 = default)
 * and panel i's exchange overlaps panel i+1's Gemm.
 * On return everything is enqueued: `out` is complete in context-stream order (WG_GATHER_NONE: this rank's rows only).
 * DIM_MISMATCH as Gemm (gemm.rs:91-95) with M = P * rows(a_rows). ALIASED: `out` shares a byte with `a_rows` or with `b` (the aliasing
 * rule; checked once, in every gather mode, before anything is launched); the one-launch forms also refuse `a_rows` / `b` views that lie in the communicator's staging cube
 * (wg_comm_stage_reserve hands that buffer out) where this rank's panels of the step are written ("Gemm: `out` overlaps `m1`" / "`m2`") -- operands elsewhere in the cube are legal.
 */
int wg_gemm_sharded(wg_comm *comm, wg_gemm_variant variant, wg_dtype dtype, wg_gather_mode mode, uint32_t panel_cols,
                    wg_buf *out, wg_view_shape out_shape,
                    const wg_buf *a_rows, wg_view_shape a_shape, const wg_buf *b, wg_view_shape b_shape);
/* The same with the N-panels' widths given one by one (`npanels` column counts, multiples of 4 summing to N): a TAPERED TAIL -- equal panels, then a
 * few narrower and narrower ones -- leaves only a narrow last panel's exchange exposed at the end of a step, and every panel's exchange still hides
 * under the next panel's Gemm as long as a panel is at least (exchange time / Gemm time) of the one before it. The one-launch forms
 * (wg_comm_set_one_launch) take lists of the shape "n equal panels of whole 256-column tiles, then 1 .. 8 other panels of whole tiles, the last one
 * whatever is left"; any other list runs panel by panel. Results are bit for bit those of wg_gemm_sharded.
 * PRECONDITION the library cannot check: EVERY rank passes the same widths (and the same panel_cols to wg_gemm_sharded) -- the list is the slot layout of the
 * staging cubes the peers copy into. Ranks with different lists would write each other's slots at the wrong offsets, silently; compare the plans across ranks once
 * before the first step (bench.py does, through its control plane). */
int wg_gemm_sharded_panels(wg_comm *comm, wg_gemm_variant variant, wg_dtype dtype, wg_gather_mode mode, const uint32_t *panel_widths, uint32_t npanels,
                           wg_buf *out, wg_view_shape out_shape,
                           const wg_buf *a_rows, wg_view_shape a_shape, const wg_buf *b, wg_view_shape b_shape);

/* ------------------------------------------------------------------------------------------------ */
/* record / replay: CommandEncoder -> finish() -> CommandBuffer -> Queue::submit, as a hipGraph      */
/* ------------------------------------------------------------------------------------------------ */
/* Start recording: operator and copy calls are captured instead of executed (no sync/read/create while recording). */
int wg_encoder_begin(wg_ctx *ctx);
/* encoder.finish(): stop recording and instantiate the replayable command buffer. */
int wg_encoder_finish(wg_ctx *ctx, wg_cmdbuf **out);
/* queue.submit(Some(cmdbuf)): enqueue one replay on the context's stream. May be submitted many times. */
int wg_queue_submit(wg_ctx *ctx, wg_cmdbuf *cmdbuf);
int wg_cmdbuf_destroy(wg_cmdbuf *cmdbuf);

/* ------------------------------------------------------------------------------------------------ */
/* GpuTimestamps (wgcore timestamps.rs): begin/end-of-pass timestamps on the context's stream        */
/* ------------------------------------------------------------------------------------------------ */
int wg_timestamps_create(wg_ctx *ctx, uint32_t capacity, wg_timestamps **out); /* GpuTimestamps::new */
int wg_timestamps_destroy(wg_timestamps *ts);
int wg_timestamps_clear(wg_timestamps *ts);
/* Record the next timestamp at the current point of the stream; *index (optional) receives its slot. (write_next_timestamp, timestamps.rs:98-102) */
int wg_timestamps_write(wg_ctx *ctx, wg_timestamps *ts, uint32_t *index);
/* next_query_indices::<COUNT> (timestamps.rs:80-94): `count` consecutive slots, all or none -- *first = UINT32_MAX when they do not fit (the reference's None; no error). */
int wg_timestamps_reserve(wg_timestamps *ts, uint32_t count, uint32_t *first);
/* write_timestamp_at (timestamps.rs:108-115): the timestamp of slot `index` (< capacity) at the current point of the stream. A reserved slot never written reads 0. */
int wg_timestamps_write_at(wg_ctx *ctx, wg_timestamps *ts, uint32_t index);
uint32_t wg_timestamps_len(const wg_timestamps *ts);
/* wait_for_results_ms (timestamps.rs:226-230): block, then out_ms[i] = time of slot i relative to the first written slot (slot 0 in the begin / end use). */
int wg_timestamps_wait_for_results_ms(wg_timestamps *ts, double *out_ms, uint32_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* WGEBRA_HIP_H */
