/* egomi.h — C-ABI of libegomi.so: the MI355X (gfx950) kernels under EgoScaler's trajectory-generator
 * hot path.
 *
 * The reference has NO native/FFI boundary on this path: its boundary is the
 * Python nn.Module API of egoscaler/models/pointllm/{builder.py,model_arch.py}, which
 * egoscaler_amd/ mirrors.  This header is the boundary UNDER that API: every entry point names the
 * reference function (file:line, relative to /root/reference/egoscaler/) whose arithmetic it
 * replaces.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless marked host; caller owns all memory
 *   - no entry point allocates, synchronises or throws; work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = default stream)
 *   - return 0 (EGOMI_OK) or a negative EGOMI_E_* code; shapes are validated on the host before
 *     any launch, so a bad call never reaches the GPU
 *   - dtype arguments: EGOMI_F32 / EGOMI_BF16 (raw uint16 storage)
 *   - thread-safe for distinct streams
 *
 * This header is the single statement of the ABI: egoscaler_amd/_abi.py reads it when the library is loaded and
 * binds every prototype, both descriptor structures and the integer EGOMI_* constants from it.  Its reader is a
 * few regular expressions, not a C parser, so declarations here keep to these rules (a line it cannot read makes
 * the load fail, naming it):
 *   - prototypes: `<return type> egomi_name(<type> <name>, ...);` with one parameter per declarator, every
 *     parameter named, no function pointers, no arrays, no macros
 *   - types: int, int64_t, size_t, float, double, egomi_stream_t; (const) pointers to void, float, double, int,
 *     int32_t, int64_t, uint8_t, uint64_t and to the two descriptors; void**; const char* as a return type only
 *   - descriptor fields: `<type> name[, name...];` of the same types; the `*` belongs to the type
 *   - constants: `#define EGOMI_NAME <integer>`, negative values in parentheses
 *   - debug-only symbols (egomi_*_stamp_*) are not declared here and are not bound
 */
#ifndef EGOMI_H
#define EGOMI_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EGOMI_OK 0
#define EGOMI_E_BADARG (-1)
#define EGOMI_E_SHAPE (-2)
#define EGOMI_E_LAUNCH (-3)
#define EGOMI_E_UNSUPPORTED (-4)

#define EGOMI_F32 0
#define EGOMI_BF16 1

typedef void* egomi_stream_t;

int egomi_version(void);
const char* egomi_strerror(int code);
/* HIP's message for the most recent failed launch on this thread (diagnostics for EGOMI_E_LAUNCH) */
const char* egomi_last_launch_error(void);

/* ------------------------------------------------------------------------------------------------
 * A1  RGB-D un-projection + ordered compaction (+ optional strided subsample)
 *     replaces  data/tools/pcm_tools.py:68-96  get_points_colors
 *     (frame loop / rgbd concat: vis/interactive.py:22-32, data/train/7_get_object_trajectory.py:244-253)
 *
 * rgb   u8  [B,T,H,W,3]      depth f32 [B,T,H,W]
 * boxes i32 [n_boxes,4] = (ymin,ymax,xmin,xmax) pixels masked out in every frame (may be NULL)
 * x = (u - pp)/fx * z,  y = (v - pp)/fy * z  in float64 exactly as numpy evaluates it;
 * colour = float32(c)/255.0f; valid = all(rgb != 0) & outside boxes & (z < d_thres).
 * d_thres = NaN disables the depth test (d_thres=None in the reference).
 * Output order is the index contract: frame-major, then row-major pixel order, valid pixels only.
 *   n_out == 0 : write every valid pixel  -> out_points f64 [B,cap,3], out_colors f32 [B,cap,3],
 *                cap = T*H*W rows reserved per sample; out_count[b] = n_valid
 *   n_out  > 0 : first-N strided subsample (stride = floor(n_valid / n_out), rows j*stride),
 *                cap = n_out; a sample with n_valid < n_out sets out_count[b] = -n_valid and its
 *                rows are left untouched (the host mirror raises ValueError).  Up to 62.9 M pixels per sample in
 *                this form (the chunk prefix lives in LDS); larger frames return EGOMI_E_UNSUPPORTED
 * Two launches (validity bits + in-chunk ranks + chunk counts; then one thread per output row, or a coalesced
 * dense writer): the workspace holds 2 x 2 B per 16 pixels + 4 B per 4096-pixel chunk per sample.
 */
size_t egomi_unproject_workspace_bytes(int B, int T, int H, int W);
int egomi_unproject_gather(const uint8_t* rgb, const float* depth, const int32_t* boxes, int n_boxes,
                           int B, int T, int H, int W, double pp, double fx, double fy, float d_thres,
                           int n_out, double* out_points, float* out_colors, int32_t* out_count,
                           void* workspace, size_t workspace_bytes, egomi_stream_t stream);

/* N4  depth map -> dense cloud: everything DepthAnything.get_depth does after the network.
 *     replaces  data/third_party/Depth-Anything-V2/metric_depth/depth.py:46-60 (get_depth) and :27-31 (get_only_depth),
 *     called from data/train/7_get_object_trajectory.py:101-108
 * pred f32 [B,h0,w0] network output, rgb u8 [B,H,W,3] (may be NULL when out_points is NULL), tab_ws i32 [W+H] scratch
 * out_z f32 [B,H,W] = PIL Image.resize((W,H), NEAREST) of pred (Pillow's running-double index walk, bit-exact);
 * out_points f64 [B,H*W,3] = ((u-pp)/fx*z, (v-pp)/fy*z, z), out_colors f64 [B,H*W,3] = rgb/255.0 — both or neither;
 * the reference returns no cloud unless fx, fy, pp > 0 (depth.py:53): asking for one with such intrinsics is BADARG. */
int egomi_depth_to_cloud(const float* pred, int B, int h0, int w0, const uint8_t* rgb, int H, int W,
                         double fx, double fy, double pp, int32_t* tab_ws,
                         float* out_z, double* out_points, double* out_colors, egomi_stream_t stream);

/* A2  pc_norm: centre xyz on the centroid, divide by the largest radius, in float64; colours pass
 *     through.   replaces  models/pointllm/pointllm/data/utils.py:146-157
 * points f64 [B,N,3], colors f32 [B,N,3] -> out f32 [B,N,6] */
int egomi_pc_norm(const double* points, const float* colors, float* out, int B, int N, egomi_stream_t stream);

/* A3  farthest point sampling.   replaces  models/pointllm/pointllm/model/pointbert/misc.py:40-60
 * pts f32 [B,N,C] (xyz = first 3 channels, C>=3), start i32 [B] (the reference draws it from the
 * global torch RNG, misc.py:52) -> out_idx i32 [B,G], out_center f32 [B,G,3].
 * fp32, d = (dx*dx+dy*dy)+dz*dz, running min from 1e10, arg-max with the LOWEST index on ties:
 * indices are bit-exact with the reference.  N <= 16384. */
int egomi_fps(const float* pts, int B, int N, int C, const int32_t* start, int G,
              int32_t* out_idx, float* out_center, egomi_stream_t stream);

/* A4+A5  kNN grouping.   replaces  pointbert/dvae.py:107-140 (square_distance, knn_point) and
 *        dvae.py:150-187 (Group.forward gather, centre subtraction on xyz only)
 * pts f32 [B,N,C], center f32 [B,G,3] -> out_idx i32 [B,G,K] ordered by (distance, index)
 * ascending, out_nb [B,G,K,C] (dtype out_dtype).  dist = ((-2*dot)+|c|^2)+|p|^2 in fp32 with
 * dot = (cx*px+cy*py)+cz*pz; no [G,N] matrix touches HBM.  N <= 8192, K <= 64. */
int egomi_knn_group(const float* pts, const float* center, int B, int N, int C, int G, int K,
                    int32_t* out_idx, void* out_nb, int out_dtype, egomi_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Dense products (MFMA).  replaces the aten linear/matmul calls inside
 *   pointbert/dvae.py:193-204 (1x1 convs, A6), pointbert/point_encoder.py:14-18,38-40 (A8),
 *   model/pointllm.py:67-81 (point_proj, A9), HF modeling_llama.py:174-176,243-281 (A11),
 *   model/pointllm.py:187,227-228 (lm_head, A12) and their autograd backward.
 *
 *   C[M,N] = act(alpha * A.B + bias) + residual  (+ C when accumulate)
 * a_layout 0: A is [M,K] row-major;  1: A is [K,M]
 * b_layout 0: B is [N,K] row-major (nn.Linear weight); 1: B is [K,N]
 * ab_dtype F32 (exact fp32 MFMA) or BF16 (fp32 accumulate); c_dtype F32 or BF16 (F32 inputs need
 * F32 output).  bias [N] has ab_dtype; residual [M,N] (ldr) has c_dtype.  act: 0 none, 1 GELU(erf),
 * 2 ReLU.  Batched: grid z in [0,batch): z0 = z / batch_inner, z1 = z % batch_inner, operand
 * pointers advance by z0*s?0 + z1*s?1 ELEMENTS (residual uses C's strides).
 */
typedef struct egomi_gemm_desc {
    const void* A; const void* B; void* C; const void* bias; const void* residual;
    int M, N, K;
    int64_t lda, ldb, ldc, ldr;
    int a_layout, b_layout;
    int ab_dtype, c_dtype;
    int batch, batch_inner;
    int64_t sA0, sA1, sB0, sB1, sC0, sC1;
    float alpha;
    int accumulate;
    int act;
    int force_generic;   /* 1: never take the tuned kernel (used by tests to cross-check it) */
    /* optional fp32 scratch.  Skinny products (M <= 512, e.g. single-token decode): split-K slabs of split_k * M * N * 4
     * bytes; split_k 0 = chosen by the library from the tile count.  Large products (256x256 kernel): the last tile rows
     * are cut into K-slices so the ragged last round fills the chip; their slabs live here too (split_k 0 = planned by
     * the library, rows*16+S = explicit).  NULL = neither. */
    void* workspace; int64_t workspace_bytes; int split_k;
    /* 1: the first 4096 bytes of `workspace` are ticket words that were ZERO when the caller first handed the buffer over and
     * are touched by nobody else; every completed launch leaves them zero again.  With this promise (and workspace_bytes >=
     * 4096 + CUs * 2 * 256 KiB) large products run the PERSISTENT form of the 256x256 kernel: one block per CU walks whole
     * tiles, the remainder of the last round is shared K-slice-wise and summed inside the launch by the last block to
     * arrive (no second kernel, nobody waits).  1: the promise is made, the library decides (today it keeps the per-tile
     * kernel: with weights cold from HBM the persistent form measured 5 % slower in the training step, csrc/gemm_fast.hip);
     * 2: the promise is made and the persistent form is taken for every shape it can run.  0: no promise. */
    int ws_tickets_zeroed;
    /* fused epilogue.  EGOMI_EPI_SWIGLU: B is [Wgate;Wup] stacked with its rows interleaved in blocks of 32 (row 64g+c =
     * Wgate[32g+c], row 64g+32+c = Wup[32g+c]); C [M,N] receives gate|up in that interleaved-32 layout (kept for backward)
     * and C2 [M, N/2] (row stride ldc2) receives silu(gate)*up = what egomi_swiglu_il_fwd(C) would write, bit for bit
     * (replaces the separate pass over C of HF LlamaMLP.forward, modeling_llama.py:174-176).  bf16 output, N % 256 == 0, no
     * bias / residual / activation / alpha / accumulate, products large enough for the 256x256 kernel
     * (egomi_gemm_kernel_id == 2); anything else returns EGOMI_E_UNSUPPORTED.
     * EGOMI_EPI_SWIGLU_BWD: the product A.B^T [M,N] is d(act), the gradient of silu(gate)*up (the data gradient of down_proj); it is never
     * stored.  C2 [M, 2N] (row stride ldc2) holds gate|up in the interleaved-32 layout (read), C [M, 2N] (row stride ldc) receives
     * d(gate|up) in the same layout = what egomi_swiglu_il_bwd would write from the stored bf16 d(act), bit for bit (replaces autograd's
     * backward of modeling_llama.py:174-176 and a round trip of d(act) through HBM).  bf16, N % 64 == 0, same restrictions as above.
     * EGOMI_EPI_SLABS: skinny split-K products (M <= 512, the single-token decode projections) leave their fp32 K-slice slabs
     * [slices][M][N] (row stride N) in `workspace` UNSUMMED and never touch C: the caller's next kernel (egomi_slabs_rmsnorm,
     * egomi_qkv_finish) sums them in slice order while doing its own work, which saves the combine pass and a round trip of the
     * product through HBM.  Plain product only (no bias / residual / activation / alpha / accumulate; add the residual in the
     * consumer), N % 4 == 0.  egomi_gemm_slab_count(desc) tells how many slices the library will write for this descriptor
     * (0: it would not split this product — use EGOMI_EPI_NONE); a request it cannot honour returns EGOMI_E_UNSUPPORTED. */
    int epilogue; void* C2; int64_t ldc2;
} egomi_gemm_desc;
#define EGOMI_EPI_NONE 0
#define EGOMI_EPI_SWIGLU 1
#define EGOMI_EPI_SLABS 2
#define EGOMI_EPI_SWIGLU_BWD 3
int egomi_gemm(const egomi_gemm_desc* desc, egomi_stream_t stream);
/* which kernel egomi_gemm would run for this descriptor: 2 = the 8-phase bf16 NT kernel (256x256 tiles, per-tile or persistent, or the
 * 352x256 form below), 1 = 128x128 / 256x128 bf16 NT kernel, 0 = generic */
int egomi_gemm_kernel_id(const egomi_gemm_desc* desc);
/* 352x256 form of the 8-phase kernel (gemm_nt_bf16_tall_kernel): whole rounds where 256x256 tiles leave a ragged last one (M = 5536, N = 4096:
 * 16 x 16 = 256 tiles instead of 22 x 16 = 352).  mode 0 = never, 1 = by the library's round model (default) — the whole product in this form, or
 * its first Na columns in this form and the rest on 256x256 tiles where neither fits alone (gate|up, the down_proj data gradient) —, 2 = the whole
 * product wherever the form applies (M % 8 == 0, N % 8 == 0, M >= 352, K >= 2048; plain, EGOMI_EPI_SLABS, EGOMI_EPI_SWIGLU, EGOMI_EPI_SWIGLU_BWD),
 * -1 = back to EGOMI_GEMM_TALL / the default.  A product that takes this form whole has no K-sliced tail rows (egomi_gemm_tail_plan: slices = 0).
 * Whole tiles are bit-identical to the 256x256 form's (same K order per element), fused epilogues included.
 * Process-wide, not thread-safe: measurement and tests only.  No reference counterpart (torch.nn.Linear's GEMM is the vendor library's). */
int egomi_gemm_set_tall(int mode);
/* The tile choice of the bf16 NT kernels, as EGOMI_GEMM_TILE sets it for a whole process: 1 = 128x128, 2 = 256x128, 8 = the 256-row forms whatever the
 * product's size (tests reach those kernels at shapes of a few tiles with it), 0 = the library's rule, -1 = back to EGOMI_GEMM_TILE / the rule.
 * Process-wide, not thread-safe: measurement and tests only.  No reference counterpart. */
int egomi_gemm_set_tile(int tile);
/* L2 touch of the 352x256 and the 256x256 per-tile kernels: in tile step t a block reads 4 bytes of each 128-B line of K-tile min(t + d, last) of its
 * A and B panels and throws them away, so that the LDS-DMA of that tile hits in L2.  Decided per launch AFTER the route and no part of it; results are
 * bit for bit the same at every d.  d = -1: back to EGOMI_GEMM_L2PF / the library's rule (default), 0 = off (the kernels run as without the feature),
 * 1..8 = that distance in every launch.  Process-wide, not thread-safe: measurement and tests only.  No reference counterpart. */
int egomi_gemm_set_l2_prefetch(int d);
/* Host-only query, launches nothing: the byte offsets those touches would read for this descriptor's M, N, K, lda, ldb and b_layout in the 352x256 form
 * (tall != 0; b_layout 1 = k-major B, N % 256 == 0) or the 256x256 per-tile form (tall == 0, b_layout 0) at distance dist, over every tile, wave, lane and
 * tile step.  out4 = {min, max offset into A, min, max into B} of the first of the 4 bytes a lane reads; -1 where nothing is touched (dist = 0). */
int egomi_gemm_l2pf_span(const egomi_gemm_desc* desc, int tall, int dist, int64_t* out4);
int egomi_gemm_slab_count(const egomi_gemm_desc* desc);   /* EGOMI_EPI_SLABS: slices egomi_gemm will leave for this descriptor, 0 = none */
/* EGOMI_EPI_SLABS on a LARGE product (egomi_gemm_kernel_id == 2): whole 256-row tiles get the normal epilogue (residual
 * included); the K-sliced tail rows [row0, M) are left as `slices` fp32 slabs [slices][M - row0][N] at the start of the slab
 * area (workspace + 4096 when ws_tickets_zeroed) for egomi_rmsnorm_fwd_tail / egomi_rmsnorm_bwd_tail to sum.  bf16 output, no
 * bias / activation / alpha / accumulate.  slices = 0: the plan has no tail rows, nothing is pending. */
int egomi_gemm_tail_plan(const egomi_gemm_desc* desc, int* row0, int* slices);
/* Query only, for k-major products (egomi_gemm_kernel_id == 3: the weight / data gradients of nn.Linear's backward, train.py:183): the
 * rows [row0, M) egomi_gemm will compute as `slices` K-slices and sum in its own combine pass (ragged last round of 256x256 tiles);
 * slices = 0: none.  EGOMI_E_UNSUPPORTED when the descriptor does not take that kernel. */
int egomi_gemm_tn_tail_plan(const egomi_gemm_desc* desc, int* row0, int* slices);
/* The route the calling thread's most recent egomi_gemm took, as its launch functions recorded it (tests: a case asserts the form it was
 * written for).  Returns the form code; out4 = {split-K slices (1 = none), first K-sliced tail row (M = none), tail slices (0 = none),
 * column split Na (0 = none)}.  Form codes:
 *   0 none (no egomi_gemm on this thread yet, or the last one launched nothing)   1 generic (gemm.hip)
 *   2 128x128 (+ skinny split-K)     3 256x128     4 gemv_m16 (M <= 16)     5 m256 ring (128 < M <= 256)
 *   6 256x256 8-phase, per tile (+ K-sliced tail rows)     7 256x256 8-phase, persistent     8 352x256
 *   9 column split: 352x256 on columns [0, Na), 256x256 per tile on the rest
 *  10 k-major 256x256 (gemm_tn.hip)     11 k-major 352x256     12 k-major column split (352x256 on [0, Na), 10 on the rest) */
int egomi_gemm_last_route(int* out4);
#define EGOMI_ROUTE_FORMS 13
/* Measurement hooks (bench.py `roofline`; no reference counterpart).  egomi_gemm_time_next(start, stop): the NEXT egomi_gemm call
 * of this thread, if it takes the 256x256 kernel (egomi_gemm_kernel_id == 2), records `start` right before and `stop` right after
 * THAT kernel on the launch stream — the slab-combine pass of K-sliced tail rows is a separate kernel and lies outside the
 * bracket; any other path leaves both events untouched.  The request is consumed by that call either way.  Events come from
 * egomi_event_create (timing-enabled HIP events); egomi_event_elapsed_ms waits for `stop`. */
int egomi_event_create(void** event);
int egomi_event_destroy(void* event);
int egomi_event_elapsed_ms(void* start, void* stop, float* ms);
int egomi_gemm_time_next(void* start, void* stop);

/* ------------------------------------------------------------------------------------------------
 * Fused attention (bf16, head_dim 128; forward also head_dim 64): softmax(scale * Q.K^T + mask).V without materialising the
 * [S,S] scores.  replaces HF eager_attention_forward, transformers/models/llama/modeling_llama.py:
 * 191-214, and its autograd backward (A11).
 * q/k/v: rows = b*S + s, row stride ld_qkv elements, head h at column h*head_dim (q, k, v may be
 * three column slices of one [B*S, 3*H*hd] buffer).  o: [B*S, H*hd] row stride ld_o.
 * mask: key j visible to query i iff (!causal || j <= i) && (key_mask == NULL || key_mask[b*S+j]).
 * lse [B,H,S] fp32 = log sum exp of the scaled, masked scores (saved for backward).
 * backward: delta [B,H,S] fp32 = rowsum(dout * o) (egomi_attn_bwd's dQ kernel computes it into `delta`, its dK/dV kernel reads it), then
 * dq/dk/dv written with row stride ld_dqkv (deterministic: no atomics).
 */
typedef struct egomi_attn_desc {
    const void* q; const void* k; const void* v; void* o; float* lse;
    const void* dout; float* delta; void* dq; void* dk; void* dv;
    const uint8_t* key_mask;
    int B, H, S, head_dim;
    int64_t ld_qkv, ld_o, ld_dqkv;
    float scale;
    int causal;
    int dtype;
    /* optional, backward only: q and k were rotated (HF apply_rotary_pos_emb, modeling_llama.py:139-167) before the
     * attention; when both tables are given (fp32 [>= S, head_dim/2], row = position s), egomi_attn_bwd writes dq and dk
     * already rotated back (what egomi_rope(..., inverse=1) on the bf16 dq/dk would give, bit for bit), so the caller
     * drops that pass.  NULL = plain dq/dk. */
    const float* rope_cos; const float* rope_sin;
    /* optional query window: 0 = every row.  0 < q_rows < S: the caller reads o and lse only at rows s >= S - q_rows of every sequence and
     * passes dout == 0 at rows s < S - q_rows.  o and lse at rows >= S - q_rows, and dq, dk, dv at EVERY row, then equal the q_rows = 0
     * call on the same inputs (dq is zero below the window); o and lse below the window are unspecified (written or left alone).  The
     * kernels only skip whole (query block, key block) pairs; every delta word the dK/dV kernel reads is written by the same call.
     * q_rows >= S behaves as 0; head_dim 64 and the first / second kernel forms may ignore it (they compute everything). */
    int q_rows;
} egomi_attn_desc;
int egomi_attn_fwd(const egomi_attn_desc* desc, egomi_stream_t stream);
int egomi_attn_bwd(const egomi_attn_desc* desc, egomi_stream_t stream);
/* A/B switch (like the EGOMI_* environment switches): 1 = the first form of the forward kernel, 2 = the round-3 instruction stream
 * (bit-identical to 1: tests/test_gpu_kernels.py), 3 = the round-4 restructure (32-key tiles in a 4-stage ring, QK of tile t+1 under the
 * exponentials of tile t, lazy running max, end-aligned query blocks; same tolerances vs fp32, not the same bits as 1 / 2), 4 = form 3 in
 * persistent blocks (default at head_dim 128 and S <= 1024: two resident blocks per CU walk the work items as one continuous K/V stream,
 * the next item's Q fragments and key mask prefetched; bit-identical to 3).
 * Process-wide, not thread-safe: measurement and tests only. */
int egomi_attn_set_fwd_form(int form);
int egomi_attn_set_fwd_blocks(int blocks);  /* form 4: cap the number of persistent blocks (0 = two per CU): tests reach several items per block at small shapes */
int egomi_attn_set_fwd_group(int group);   /* block order of form 3: 0 = rank-major, G = a (b,h) pair's blocks in groups of G ranks on one XCD */
int egomi_attn_set_bwd_form(int form);   /* likewise for the two backward kernels */

/* Consumers of EGOMI_EPI_SLABS products (single-token decode; replace splitk combine + the next elementwise kernels of
 * HF LlamaDecoderLayer.forward, modeling_llama.py:243-281, with identical rounding).  slabs: fp32 [slices][rows][cols].
 * egomi_slabs_rmsnorm: x_out = round(sum slabs + residual), h_out = rmsnorm(x_out) * w          (cols % 8 == 0, <= 8192)
 * egomi_qkv_finish   : q|k|v = round(sum slabs) [B, 3*H*hd]; RoPE(pos) on q, k; q -> qkv (row stride ld), k, v -> caches
 *                      [B,H,Smax,hd] at position pos */
int egomi_slabs_rmsnorm(const float* slabs, int slices, int rows, int cols, const void* residual, int64_t ldr, const void* w, float eps,
                        void* x_out, int64_t ldx, void* h_out, int64_t ldh, int dtype, egomi_stream_t stream);
int egomi_qkv_finish(const float* slabs, int slices, void* qkv, int64_t ld, const float* cos_tab, const float* sin_tab, int pos,
                     void* kcache, void* vcache, int B, int H, int hd, int Smax, int dtype, egomi_stream_t stream);
/* ------------------------------------------------------------------------------------------------
 * A13  cached decoding.  replaces the past_key_values branch of HF LlamaAttention.forward
 * (modeling_llama.py:243-281) and the greedy step of generate (models/pointllm/model_arch.py:94-108,
 * pointllm/model/pointllm.py:255-275).  KV cache layout [B, H, Smax, hd] per layer (contiguous
 * per-(batch, head) streams).  No entry point reads a length from device memory: every step's
 * constants are arguments, so a whole multi-step decode can be captured into one hipGraph.
 *   kv_append : k, v rows [B*S, H*hd] (row stride ld) -> cache[b, h, pos0+s, :]
 *   attn_decode: q [B, H*hd] against keys [0, T_len) -> out [B, H*hd]; key_mask [B, >=T_len] u8 or NULL.  One kernel
 *                (csrc/attn_decode.hip) serves this entry point, attn_decode_rows and the two fp8 forms below.
 *   argmax_rows: ids[b] = argmax logits[b, :] (lowest index on ties); seq[b*ld_seq + pos] = ids[b]
 */
int egomi_kv_append(const void* k, const void* v, int64_t ld, void* kcache, void* vcache, int B, int S, int H, int hd, int Smax,
                    int pos0, int dtype, egomi_stream_t stream);
int egomi_attn_decode(const void* q, int64_t ld_q, const void* kcache, const void* vcache, const uint8_t* key_mask, int64_t ld_mask,
                      void* out, int64_t ld_o, int B, int H, int hd, int Smax, int T_len, float scale, int dtype,
                      egomi_stream_t stream);
int egomi_argmax_rows(const void* logits, int64_t ld, int B, int V, int64_t* ids, int64_t* seq, int64_t ld_seq, int pos, int dtype,
                      egomi_stream_t stream);
/* sample_rows: everything HF GenerationMixin.generate does between two forward passes under the arguments the reference passes
 * (models/pointllm/model_arch.py:82-108: do_sample=True, top_k=50, top_p=0.95, temperature, repetition_penalty,
 * output_scores=True, return_dict_in_generate=True; train.py:223-228 validates this way), for a whole batch in one launch:
 *   scores[b, :] = TopP(TopK(Temperature(RepetitionPenalty(logits[b, :]))))   fp32, -inf where a warper removed the token
 *                  (transformers/generation/logits_process.py: RepetitionPenaltyLogitsProcessor on the tokens seq[b, rep_from:pos],
 *                  TemperatureLogitsWarper, TopKLogitsWarper — ties with the k-th value kept —, TopPLogitsWarper — ascending stable
 *                  order, prefix with cumulative probability <= 1 - top_p removed, min_tokens_to_keep = 1)
 *   ids[b]       = do_sample ? a draw from softmax(scores[b, :]) (Gumbel-max on Philox4x32-10 bits keyed by rng[0] = seed and
 *                  rng[1] + draw = draw counter, both read from DEVICE memory at run time so that a replayed hipGraph draws fresh
 *                  numbers; replaces torch.multinomial, whose stream cannot be reproduced) : argmax (lowest index on ties)
 *   done[b]      (may be NULL) HF's unfinished_sequences: a finished row emits pad_id, a row finishes when it emits eos_id (< 0: never)
 *   seq[b*ld_seq + pos] = ids[b]  (may be NULL)
 * top_k = 0 / top_p = 1 / temperature = 1 / repetition_penalty = 1 switch the respective step off.  `pos`, `draw` are launch
 * constants (no length is read from device memory), so T steps can be captured into one hipGraph. */
int egomi_sample_rows(const void* logits, int64_t ld, int B, int V, float* scores, int64_t ld_scores, int64_t* seq, int64_t ld_seq,
                      int pos, int rep_from, int64_t* ids, int* done, float repetition_penalty, float temperature, int top_k,
                      float top_p, int do_sample, const uint64_t* rng, int draw, int64_t eos_id, int64_t pad_id, int dtype,
                      egomi_stream_t stream);
/* token_logprob / seq_rank: which of K sampled sequences the model itself finds most probable (csrc/logprob.hip).  Replaces
 * transformers/generation/utils.py compute_transition_scores on generate(output_logits=True): log_softmax of the RAW logits of every
 * step, gathered at the chosen token and summed per sequence -- without keeping [T, rows, V] raw logits or leaving the captured loop.
 *   token_logprob: one launch per decode step, after sample_rows / argmax_rows wrote tok; reads the logits they read (bf16 or fp32 [R, V],
 *                row stride ld >= V).  Per row r: live != NULL and live[r] == 0 -> tok_lp[r*ld_lp + col] = 0, nothing else.  Otherwise
 *                m = max x, s = sum exp(x - m) (fp32, in an order that depends on V only: a row's bits do not depend on R, its slot or its
 *                alignment), lp = (x[tok[r]] - m) - log s (accurate expf / logf); tok_lp[r*ld_lp + col] = lp, sum_lp[r] += lp,
 *                n_tok[r] += 1; then, with live != NULL, eos_id >= 0 and tok[r] == eos_id, live[r] = 0: the eos is counted, the pads after
 *                it are not, also when pad == eos (the kernel does not read sample_rows' `done`, already set for this step).
 *                live == NULL: every row counts at every step.  The caller zeroes sum_lp / n_tok and sets live = 1 before step 0.
 *                tok[r] outside [0, V) is device data, so no code reports it: the row's lp is NaN (x[clamp(tok)] is what is read; the
 *                NaN reaches tok_lp, sum_lp and every score ranked from it).  `col` is a launch constant; no atomics; a replay is bit-equal.
 *                Returns BADARG (NULL logits / tok / tok_lp / sum_lp / n_tok, unknown dtype), SHAPE (R, V <= 0, ld < V, col outside
 *                [0, ld_lp)), UNSUPPORTED (logits not aligned to their element size).
 *   seq_rank   : sum_lp, n_tok [B*K] -> score[b*K + j] = sum_lp / powf(n_tok, length_penalty) (HF's beam convention: 1 = mean
 *                log-prob, 0 = the sum; n_tok == 0 -> -inf) and order[b, :] = the clip's K indices by descending score, ties -> lower
 *                index, -inf rows last in index order (a NaN score ranks as -inf).  BADARG (NULL, NaN penalty), SHAPE (B, K <= 0),
 *                UNSUPPORTED (K > 1024). */
int egomi_token_logprob(const void* logits, int64_t ld, int R, int V, const int64_t* tok, int64_t eos_id, int32_t* live, float* tok_lp,
                        int64_t ld_lp, int col, float* sum_lp, int32_t* n_tok, int dtype, egomi_stream_t stream);
int egomi_seq_rank(const float* sum_lp, const int32_t* n_tok, int B, int K, float length_penalty, float* score, int32_t* order,
                   egomi_stream_t stream);
/* bin_stats: the step's distribution over the waypoint bins (csrc/logprob.hip).  Token ids p0 .. p0 + nb - 1 stand for the values
 * values[0 .. nb-1] (float64 [nb], device memory: numpy.linspace(-1, 1, nb) for the trajectory tokens, the table the A14 entry points
 * take as `bins`).  One launch per decode step on the RAW logits token_logprob reads (bf16 or fp32 [R, V], row stride ld >= V); it keeps
 * no state and reads no token, so it may run anywhere after the logits exist.  Per row: m = max x, s = sum exp(x - m) over all V
 * (token_logprob's pass, the same code); w_i = exp(x[p0 + i] - m) in fp32 (-inf -> 0), Z = sum w_i, and in float64, in a fixed order:
 *   mass[r*ld_out + col] = Z / s                          the probability that the step's token is a bin token at all
 *   mean[r*ld_out + col] = sum w_i v_i / Z                E[v | bin]
 *   std [r*ld_out + col] = sqrt(sum w_i (v_i - mean)^2 / Z)   (the centred second pass, not E[v^2] - mean^2)
 *   ent [r*ld_out + col] = -sum q_i log q_i, q_i = w_i / Z, 0 log 0 = 0, in nats
 * all stored as fp32.  Every bin -inf (Z = 0): mass = 0, mean = std = ent = NaN.  A NaN logit anywhere in the row: mass = NaN; inside
 * the window: all four NaN.  Nothing outside [row, row + V) is read.  `col` is a launch constant; no atomics; a row's bits depend on
 * (V, p0, nb, dtype) and its values only, not on R, its slot, its alignment or ld; a replay is bit-equal.
 * Returns BADARG (a NULL pointer, unknown dtype), SHAPE (R, V <= 0, ld < V, nb outside 1 .. 1024, p0 < 0, p0 + nb > V, col outside
 * [0, ld_out)), UNSUPPORTED (logits not aligned to their element size). */
int egomi_bin_stats(const void* logits, int64_t ld, int R, int V, int p0, int nb, const double* values, float* mass, float* mean,
                    float* std, float* ent, int64_t ld_out, int col, int dtype, egomi_stream_t stream);
/* Constrained decoding of trajectories (csrc/grammar.hip; HF: generate(prefix_allowed_tokens_fn=...), logits_process.py
 * PrefixConstrainedLogitsProcessor, without its per-row host callback).  The grammar <ts> (bin x 6 <tsep>) x n <te> eos with
 * min_steps <= n <= max_steps over the bin ids p0 .. p0 + nb - 1 and the four special ids is a ten-state machine; a decoder row's state
 * is int32 (phase, steps), state[2 r] and state[2 r + 1].  The transition table, the allowed set of every state and need(state) are
 * stated once, in the header comment of csrc/grammar.hip.
 *   grammar_init: ids int64 [R, S0] (row stride ld_ids), mask uint8 [R, S0] (row stride ld_mask) or NULL; positions with mask == 0 are
 *                skipped.  state[r] = the state the prompt leaves (from its last <ts>: steps = the <tsep> after it, phase = the trailing
 *                run of bins, capped at 6; no <ts>: (9, 0)) and need[r] = the tokens to the earliest legal close, EGOMI_GRAMMAR_NEVER
 *                where the prompt already holds more steps than max_steps.  A row with need <= T_new ends `<te> eos` inside T_new steps.
 *   grammar_step: one launch per decode step directly before the token kernel, in place on the logits (bf16 or fp32 [R, V], row stride
 *                ld).  Per row: tok_prev != NULL advances state[r] by tok_prev[r] (a token the state does not allow leaves it as it
 *                is); mass[r*ld_mass + col] = sum exp(x_a - m) over the allowed ids / sum exp(x - m) over all V, on the RAW row
 *                (token_logprob's pass; the allowed sum in float64 in a fixed order; a NaN logit gives NaN); then -inf over every id of
 *                [0, V) that is not allowed.  rem = the tokens the loop still emits, this one included: at a step boundary a new step
 *                may open only when rem >= 9.  Allowed elements are not written, nor is any byte outside [row, row + V): padding
 *                columns and neighbouring rows stay.  Every allowed logit -inf: mass = 0 and the row ends all -inf.  rem and col are
 *                launch constants; no atomics; a row's bits depend on its values, its state and (V, spec, dtype) only; a replay is
 *                bit-equal.
 * Both return BADARG (a NULL pointer other than mask / tok_prev, unknown dtype), SHAPE (a size <= 0, a row stride below its row, rem < 1,
 * col outside [0, ld_mass), nb outside 1 .. 1024, p0 < 0, min_steps < 0 or > max_steps, a special id negative, inside the bin window or
 * equal to another; grammar_step also: the window or a special id outside [0, V)), grammar_step UNSUPPORTED (logits not aligned to
 * their element size). */
#define EGOMI_GRAMMAR_NEVER 1073741824
int egomi_traj_grammar_init(const int64_t* ids, int64_t ld_ids, const uint8_t* mask, int64_t ld_mask, int R, int S0, int64_t p0, int nb,
                            int64_t ts, int64_t tsep, int64_t te, int64_t eos, int min_steps, int max_steps, int32_t* state, int32_t* need,
                            egomi_stream_t stream);
int egomi_traj_grammar_step(void* logits, int64_t ld, int R, int V, const int64_t* tok_prev, int32_t* state, int64_t p0, int nb, int64_t ts,
                            int64_t tsep, int64_t te, int64_t eos, int min_steps, int max_steps, int rem, float* mass, int64_t ld_mass, int col,
                            int dtype, egomi_stream_t stream);
/* Motion limits in constrained decoding: the two grammar kernels with a per-row table of limits and a per-row pose (csrc/grammar.hip states
 * the one rule).  lim int32 [R, 18] = lo[6] | hi[6] | dmax[6] in bins: the inclusive box per trajectory dimension and the largest allowed
 * |bin_t - bin_(t-1)|, nb - 1 = no cap.  pose int32 [R, 12] = prev[6] | cur[6]: the bins of the last CLOSED step (-1: unknown) and of the
 * open step seen so far.  Both are contiguous.
 *   grammar_init_limits: grammar_init, and pose[r] from the prompt: prev is committed at a <tsep> only when the run before it held six
 *                bins (else -1), <ts> resets it, cur = the bins of the trailing run (-1 elsewhere).  No <ts>: all -1.
 *   grammar_step_limits: grammar_step, where the state allows bins at phase p with the window of bin ids narrowed to dimension p's
 *                [max(lo, q - dmax), min(hi, q + dmax)] around q = prev[p] ([lo, hi] when q < 0; when that is empty, q lies farther than
 *                dmax outside the box and the one bin dmax nearer to the box is the window).  Never empty, always inside the bin ids:
 *                lo, hi, dmax and q are clamped into range on load, so the kernel is safe on a table nobody checked (the launch cannot
 *                read it; decode.traj_limits_check does on the host).  tok_prev moves the pose with the state: a bin taken at phase p
 *                sets cur[p], <tsep> taken at phase 6 copies cur to prev, <ts> taken at phase 9 sets prev to -1, any token that does not
 *                move the phase leaves it.  mass keeps grammar_step's meaning and bits (what the grammar ALONE allows);
 *                limits_mass[r*ld_mass + col] = the same sum over the ids allowed under the limits, the same float64 terms in the same
 *                order: with a full-range table it is bit-equal to mass, and so are the logits and the state to grammar_step's.  A
 *                row's bits depend on its values, state, pose, limits and (V, spec, dtype) only.
 * Errors as grammar_init / grammar_step; pose, lim and limits_mass NULL: BADARG. */
int egomi_traj_grammar_init_limits(const int64_t* ids, int64_t ld_ids, const uint8_t* mask, int64_t ld_mask, int R, int S0, int64_t p0, int nb,
                                   int64_t ts, int64_t tsep, int64_t te, int64_t eos, int min_steps, int max_steps, int32_t* state,
                                   int32_t* need, int32_t* pose, egomi_stream_t stream);
int egomi_traj_grammar_step_limits(void* logits, int64_t ld, int R, int V, const int64_t* tok_prev, int32_t* state, int64_t p0, int nb,
                                   int64_t ts, int64_t tsep, int64_t te, int64_t eos, int min_steps, int max_steps, int rem, float* mass,
                                   int64_t ld_mass, int col, const int32_t* lim, int32_t* pose, float* limits_mass, int dtype,
                                   egomi_stream_t stream);
/* Beam search / beam sampling (num_beams > 1): HF GenerationMixin._beam_search, transformers 5.15 generation/utils.py:3208-3560.
 * Logical rows r = b * nb + j (item b, beam j), R = B * nb.  Every step is one beam_rows + one beam_update launch; ctl (int32 [6], device)
 * holds the loop-open flag [0] and the iteration count [1]: once a step closes the loop, both return at once, so T captured steps
 * replay HF's data-dependent number of iterations.
 *   beam_rows  : replaces :3347-3385 (log_softmax of fp32 logits, logits_processor on the LOG-PROBS against the row's own sequence
 *                seq[r, 0:pos], + running_beam_scores) and the per-row half of _get_top_k_continuations :3077.  Row r reads logits row
 *                r / lg_div (lg_div = nb at step 0: the item's prefill row).  scores[r, :] = the processed row (RepetitionPenalty,
 *                with do_sample also Temperature -> TopK -> TopP with min_tokens_to_keep, :1299-1305); then acc = scores + run_score[r]
 *                (+ Gumbel noise of egomi_sample_rows' Philox stream at (rng[0]; row r, token, rng[1] + draw) when sampling: Gumbel-top-K
 *                is sequential sampling without replacement from softmax(acc), torch.multinomial's role); the row's K largest keys
 *                (ties -> lower flat index j * V + token) -> cand_key (perturbed), cand_score (acc), cand_tok [R, K].
 *   beam_update: one workgroup per item: the item's top K of its nb * K candidates (_get_top_k_continuations), stopping marks (eos,
 *                cur_len + 1 >= max_len), _get_running_beams_for_next_iteration, _update_finished_beams :3153 (length penalty,
 *                early_stopping 0 False / 1 True / 2 "never"), _check_early_stop_heuristic :3007, _beam_search_has_unfinished_sequences
 *                :3055.  Gathers the parents of seq / fin_seq [R, ld_seq], beam_idx / fin_beam_idx [R, ld_bidx] (batch-offset, HF's
 *                beam_indices) and kv_row [R, ld_kv] in place (kv_row[r, cur_len] = r: the row's own physical cache row), writes tok[r],
 *                run_score, fin_score, fin_flag [R], heur [B].  Ties -> the lower position, as the kernel tests pin.
 *   attn_decode_rows: attn_decode with key t of logical row r read from physical row kv_row[r, t] of the [n_phys, H, Smax, hd] caches
 *                (the reorder of the cache by parent beam, :3437-3447, as a table gather: no K/V bytes move); key_mask [R, >= T_len]. */
int egomi_beam_rows(const void* logits, int64_t ld, int lg_div, int R, int V, int nb, float* scores, int64_t ld_scores, const int64_t* seq,
                    int64_t ld_seq, int pos, float repetition_penalty, float temperature, int top_k, float top_p, int min_tokens_to_keep,
                    int do_sample, const uint64_t* rng, int draw, const float* run_score, int K, float* cand_key, float* cand_score,
                    int32_t* cand_tok, const int32_t* ctl, int dtype, egomi_stream_t stream);
int egomi_beam_update(int B, int nb, int K, int V, const float* cand_key, const float* cand_score, const int32_t* cand_tok, int S0, int cur_len,
                      int max_len, int64_t eos_id, float length_penalty, int early_stopping, int64_t* seq, int64_t* fin_seq, int64_t ld_seq,
                      int32_t* beam_idx, int32_t* fin_beam_idx, int64_t ld_bidx, int32_t* kv_row, int64_t ld_kv, float* run_score,
                      float* fin_score, int32_t* fin_flag, int32_t* heur, int64_t* tok, int32_t* ctl, egomi_stream_t stream);
int egomi_attn_decode_rows(const void* q, int64_t ld_q, const void* kcache, const void* vcache, const int32_t* kv_row, int64_t ld_kv,
                           int n_phys, const uint8_t* key_mask, int64_t ld_mask, void* out, int64_t ld_o, int B, int nb, int H, int hd,
                           int Smax, int T_len, float scale, int dtype, egomi_stream_t stream);
/* Shared-prompt decode attention (csrc/shared.hip): best-of-K sampling without HF's _expand_inputs_for_generation (generation/utils.py,
 * reached from models/pointllm/model_arch.py:94-108 with num_return_sequences = K), which repeats every prompt K times in the batch and
 * in the KV cache.  Logical rows r = b * K + j (clip b, sample j), 1 <= K <= 32.
 *   kprompt, vprompt [B, H, Sp, hd]     one row per CLIP, keys 0 .. S0-1; key_mask [B, >= S0] u8 (1 = visible) or NULL
 *   ksuffix, vsuffix [B*K, H, Tmax, hd] one row per logical row, keys 0 .. T_len-1 (the tokens the row generated; T_len = 0: may be NULL)
 *   out[r] = attention of q[r] over (prompt keys of clip r / K, then the row's suffix keys): what egomi_attn_decode gives on the
 *            physically concatenated cache of row r.  q [B*K, H*hd] (16-B aligned rows), out [B*K, H*hd]; a row that sees no key gives 0.
 * One workgroup per (clip, head) serves all K queries, so every prompt K/V element is loaded once per (clip, head) and launch (bf16 at
 * hd 64 / 128: MFMA; otherwise VALU over an LDS-staged tile).  Fixed summation order: replays are bit-equal, and a row's result does not
 * depend on its slot j.  dtype EGOMI_BF16 / EGOMI_F32, hd in {32, 64, 128} (EGOMI_E_UNSUPPORTED otherwise). */
int egomi_attn_decode_shared(const void* q, int64_t ld_q, const void* kprompt, const void* vprompt, const uint8_t* key_mask, int64_t ld_mask,
                             const void* ksuffix, const void* vsuffix, void* out, int64_t ld_o, int B, int K, int H, int hd, int Sp, int S0,
                             int Tmax, int T_len, float scale, int dtype, egomi_stream_t stream);
/* The suffix pass of egomi_attn_decode_shared: teacher-forced scoring of K given candidates per clip, T suffix tokens each, in ONE launch.
 * Logical query row (b * K + j) * T + t (clip b, candidate j, suffix position t); 1 <= K <= 32, 1 <= T <= Tmax, 1 <= S0 <= Sp.
 *   q [B*K*T, ld_q] (16-B aligned rows), out [B*K*T, ld_o]
 *   kprompt, vprompt [B, H, Sp, hd], key_mask [B, >= S0] u8 or NULL: as above
 *   ksuffix, vsuffix [B*K, H, Tmax, hd]: keys 0 .. T-1 of every candidate row, already appended
 *   out[(b*K + j)*T + t] = attention of that query over the visible prompt keys of clip b, then suffix keys 0 .. t of row b*K + j (causal):
 *            what egomi_attn_decode_shared gives that query at T_len = t + 1, bit for bit.  (A query always sees its own key; a fully
 *            masked prompt is legal.)
 * One workgroup per (clip, head, tile of 32 consecutive of the clip's K*T queries): the prompt K/V pass through LDS once per workgroup and
 * serve the whole tile (bf16 at hd 64 / 128: MFMA; otherwise VALU), then every query walks its own causal cut of its candidate's suffix.
 * Fixed summation order, no atomics: replays are bit-equal, and the bits of (b, j, t) depend on its own data and (S0, t, hd, dtype) only,
 * not on K, T, j, b or the queries that share its tile.  Never read: suffix keys > t or >= T, prompt keys >= S0.  Dtypes, head dims and
 * error codes are those of egomi_attn_decode_shared (T = 0, T > Tmax, more than 2^31 - 1 workgroups: EGOMI_E_SHAPE). */
int egomi_attn_suffix_shared(const void* q, int64_t ld_q, const void* kprompt, const void* vprompt, const uint8_t* key_mask, int64_t ld_mask,
                             const void* ksuffix, const void* vsuffix, void* out, int64_t ld_o, int B, int K, int H, int hd, int Sp, int S0,
                             int Tmax, int T, float scale, int dtype, egomi_stream_t stream);
/* egomi_attn_decode_shared with the suffix read through a row table: beam search on the prompt / suffix cache layout.  K = beams per clip,
 * logical row r = b * K + j; suffix key t of row r lives in physical suffix row sfx_row[r * ld_row + t] of ksuffix, vsuffix
 * [n_phys, H, Tmax, hd] (a beam's suffix is the path through its ancestors' rows; egomi_beam_update keeps the table).  An entry outside
 * [0, n_phys) is a masked key: its address is clamped and its score selected away, never dereferenced (the convention of
 * egomi_attn_decode_rows_fp8).  sfx_row [B*K, ld_row >= T_len] int32 (T_len = 0: may be NULL).  Every other argument, the result, the
 * layouts, dtypes and head dims are those of egomi_attn_decode_shared, and so is the prompt phase; each query's suffix keys are split
 * into contiguous slices over the workgroup's idle lane groups and merged in slice order (csrc/shared.hip).  Every sum has a fixed order
 * given by (K, S0, T_len): no atomics, replays are bit-equal, and permuting the beams of a clip (queries and table rows together)
 * permutes the output rows bit for bit. */
int egomi_attn_decode_shared_rows(const void* q, int64_t ld_q, const void* kprompt, const void* vprompt, const uint8_t* key_mask, int64_t ld_mask,
                                  const void* ksuffix, const void* vsuffix, const int32_t* sfx_row, int64_t ld_row, int n_phys, void* out,
                                  int64_t ld_o, int B, int K, int H, int hd, int Sp, int S0, int Tmax, int T_len, float scale, int dtype,
                                  egomi_stream_t stream);

/* FP8 (OCP e4m3fn) KV cache (csrc/kv8.hip; attention: csrc/attn_decode.hip): codes uint8 [B, H, Smax, hd] per layer (the bf16 cache's layout), scales fp32 [B, H, Smax]
 * per layer; hd in {32, 64, 128} (EGOMI_E_UNSUPPORTED otherwise); codes 8-B (attention: 16-B) aligned, scales 4-B aligned.  Per (row, head, position)
 * and tensor: s = amax / 448 (1 when amax == 0), code = e4m3fn_rne(x / s), value = float(code) * s, x being what the bf16 / fp32
 * kernel below would have stored (bit-equal to torch's (x / s).to(torch.float8_e4m3fn); see the header of csrc/kv8.hip).
 *   kv_append_fp8       : egomi_kv_append into the fp8 cache
 *   qkv_finish_fp8      : egomi_qkv_finish with k, v quantised into the fp8 cache at pos (q -> qkv bit-equal to egomi_qkv_finish)
 *   attn_decode_fp8     : egomi_attn_decode over the fp8 cache (a masked or out-of-range key is selected away, never read as 0 * code)
 *   attn_decode_rows_fp8: egomi_attn_decode_rows over the fp8 cache (kv_row entries outside [0, n_phys) are masked keys) */
int egomi_kv_append_fp8(const void* k, const void* v, int64_t ld, uint8_t* kcodes, uint8_t* vcodes, float* kscale, float* vscale, int B, int S,
                        int H, int hd, int Smax, int pos0, int dtype, egomi_stream_t stream);
int egomi_qkv_finish_fp8(const float* slabs, int slices, void* qkv, int64_t ld, const float* cos_tab, const float* sin_tab, int pos,
                         uint8_t* kcodes, uint8_t* vcodes, float* kscale, float* vscale, int B, int H, int hd, int Smax, int dtype,
                         egomi_stream_t stream);
int egomi_attn_decode_fp8(const void* q, int64_t ld_q, const uint8_t* kcodes, const uint8_t* vcodes, const float* kscale, const float* vscale,
                          const uint8_t* key_mask, int64_t ld_mask, void* out, int64_t ld_o, int B, int H, int hd, int Smax, int T_len,
                          float scale, int dtype, egomi_stream_t stream);
int egomi_attn_decode_rows_fp8(const void* q, int64_t ld_q, const uint8_t* kcodes, const uint8_t* vcodes, const float* kscale,
                               const float* vscale, const int32_t* kv_row, int64_t ld_kv, int n_phys, const uint8_t* key_mask,
                               int64_t ld_mask, void* out, int64_t ld_o, int B, int nb, int H, int hd, int Smax, int T_len, float scale,
                               int dtype, egomi_stream_t stream);

/* FP8 (OCP e4m3fn) weights of the single-token decode projections, W8A16 (csrc/w8.hip).  Replaces the bf16 q|k|v, o_proj, gate|up and
 * down_proj products of a cached decode step (HF LlamaAttention / LlamaMLP forward, modeling_llama.py:243-281,174-176, in the generate()
 * step of models/pointllm/model_arch.py:77-108 / pointllm/model/pointllm.py:255-275).  Per output row n of W [N, K]:
 * s_n = amax_k |W[n,k]| / 448 (1 when amax == 0), code[n,k] = e4m3fn_rne(W[n,k] / s_n) -- the KV cache's rule, bit-equal to torch's
 * (W.float() / s[:, None]).to(torch.float8_e4m3fn).
 *   quantize_rows_fp8: bf16 rows w [N, K] (row stride ldw) -> codes uint8 [N, K] (row stride ldc), scales fp32 [N]
 *   gemm_w8          : y[m,n] = s_n * sum_k x[m,k] * float(code[n,k]); x bf16 [M, K] (ldx % 8 == 0, 16-B aligned), codes [N, K] (ldw % 16
 *                      == 0, 16-B aligned), fp32 accumulation in a fixed order, s_n applied after accumulation (to each K-slice).
 *                      1 <= M <= 512, N % 4 == 0, K % 32 == 0 (EGOMI_E_UNSUPPORTED otherwise).  epilogue EGOMI_EPI_NONE: out bf16 [M, N]
 *                      (row stride ldo) = bf16(y), or bf16(y + residual) when residual (bf16 [M, N], row stride ldr) is not NULL; the
 *                      optional workspace lets the library split K.  EGOMI_EPI_SLABS: out and residual unused (residual must be NULL),
 *                      the fp32 slabs [slices][M][N] (sum = y) land at the start of the 16-B aligned workspace for egomi_slabs_rmsnorm /
 *                      egomi_qkv_finish(_fp8); a repeated call writes the same bits (no atomics).
 *   gemm_w8_slab_count: the number of slabs egomi_gemm_w8 writes with EGOMI_EPI_SLABS for this shape and workspace (0: it cannot run it).
 *                      Plan and launch are one function of the library. */
int egomi_quantize_rows_fp8(const void* w, int64_t ldw, int N, int K, uint8_t* codes, int64_t ldc, float* scales, egomi_stream_t stream);
int egomi_gemm_w8(const void* x, int64_t ldx, const uint8_t* codes, int64_t ldw, const float* scales, void* out, int64_t ldo,
                  const void* residual, int64_t ldr, int M, int N, int K, int epilogue, void* workspace, int64_t workspace_bytes,
                  egomi_stream_t stream);
int egomi_gemm_w8_slab_count(int M, int N, int K, int64_t workspace_bytes);

/* Int4 weights with group scales of the single-token decode projections, W4A16 (csrc/w4.hip; its header is the normative statement).
 * Replaces the same bf16 products as the fp8 form above (HF LlamaAttention / LlamaMLP forward, modeling_llama.py:243-281,174-176, in the
 * generate() step of models/pointllm/model_arch.py:77-108 / pointllm/model/pointllm.py:255-275).  Group g of a row is its columns
 * [128 g, min(K, 128 g + 128)), NG = ceil(K / 128); s[g,n] = amax / 7.0f (1 when amax == 0), code = clamp(rintf(W / s), -7, 7), stored as
 * the nibble code + 8: byte b of a row holds column 2 b in its low nibble and column 2 b + 1 in its high nibble (16 bytes per 32 columns).
 *   quantize_rows_int4: bf16 rows w [N, K] (row stride ldw, K % 32 == 0) -> packed codes uint8 [N, K / 2] (row stride ldc bytes, ldc % 4
 *                      == 0), scales fp32 [NG, N] (group-major, contiguous); bit-equal to decode.w4_quantize on the host.
 *   gemm_w4          : y[m,n] = sum_g s[g,n] * (sum_{k in g} x[m,k] * code[n,k]); x bf16 [M, K] (ldx % 8 == 0, 16-B aligned), packed codes
 *                      (ldw bytes, ldw % 16 == 0, 16-B aligned), scales 16-B aligned; fp32 accumulation in a fixed order, a group's sum is
 *                      finished before its scale is applied.  Shapes, epilogues (EGOMI_EPI_NONE with optional residual and workspace,
 *                      EGOMI_EPI_SLABS), the slabs' layout and the error codes are egomi_gemm_w8's; a repeated call writes the same bits.
 *   gemm_w4_slab_count: the number of slabs egomi_gemm_w4 writes with EGOMI_EPI_SLABS for this shape and workspace (0: it cannot run it). */
int egomi_quantize_rows_int4(const void* w, int64_t ldw, int N, int K, uint8_t* codes, int64_t ldc, float* scales, egomi_stream_t stream);
int egomi_gemm_w4(const void* x, int64_t ldx, const uint8_t* codes, int64_t ldw, const float* scales, void* out, int64_t ldo,
                  const void* residual, int64_t ldr, int M, int N, int K, int epilogue, void* workspace, int64_t workspace_bytes,
                  egomi_stream_t stream);
int egomi_gemm_w4_slab_count(int M, int N, int K, int64_t workspace_bytes);

/* LoRA adapters on the decoder projections (csrc/lora.hip): the low-rank products of PEFT's lora.Linear.forward (peft/tuners/lora/layer.py:
 * result = base_layer(x) + lora_B(lora_A(x)) * scaling, scaling = lora_alpha / r; no dropout, no bias) and of its backward.  For one adapted
 * projection with A [r, K], B [N, r] and s = lora_alpha / r: T = x A^T, y += s T B^T; U = dY B, dX += s U A, dA = s U^T x, dB = s dY^T T;
 * merging W' = W + s B A.  dtype EGOMI_F32 or EGOMI_BF16 for every operand but G; fp32 accumulation in a fixed order, no atomics.
 * il = 1: logical column c of the wide activation operand (X of lora_down, Y of lora_up, L of lora_wgrad) lies at 64 * (c / 32) + c % 32,
 * the interleaved-32 gate|up layout (its row stride must hold 2 * width - 32 columns; the up half starts 32 columns in).
 *   lora_down : y[m, j] = alpha * sum_k x[m, k] q(j, k), m < M, j < R, k < K; q(j, k) = q_trans ? q[k ldq + j] : q[j ldq + k].  Stacking n
 *               adapters that share x ([A_1; ...; A_n], R = n r) reads x once.  K is cut into fixed 512-deep slices whose fp32 partials go
 *               to `workspace` (egomi_lora_down_workspace_bytes(M, K, R) bytes; 0 = none needed) and are summed in slice order.
 *   lora_up   : y[m, n] = dtype(float(y[m, n]) + alpha * sum_j p[m, j] q(n, j)), n < N, j < R; q(n, j) = q_trans ? q[j ldq + n] : q[n ldq + j].
 *   lora_wgrad: G[p, q] = (accumulate ? G[p, q] : 0) + alpha * sum_m l[m, p] r[m, q] (G fp32 [P, Q], row stride ldg), m < M; one of P, Q
 *               at most 192.  M is cut into fixed 256-row slices whose fp32 partials go to `workspace`
 *               (egomi_lora_wgrad_workspace_bytes(M, P, Q) bytes; 0 = none needed) and are summed in slice order.
 * R (lora_down, lora_up) % 8 == 0 and 8 <= R <= 192, il with a width % 32 != 0, and other dtypes return EGOMI_E_UNSUPPORTED. */
int64_t egomi_lora_down_workspace_bytes(int M, int K, int R);
int egomi_lora_down(const void* x, int64_t ldx, const void* q, int64_t ldq, int q_trans, void* y, int64_t ldy, int M, int K, int R,
                    float alpha, int il, void* workspace, int64_t workspace_bytes, int dtype, egomi_stream_t stream);
int egomi_lora_up(const void* p, int64_t ldp, const void* q, int64_t ldq, int q_trans, void* y, int64_t ldy, int M, int N, int R, float alpha,
                  int il, int dtype, egomi_stream_t stream);
int64_t egomi_lora_wgrad_workspace_bytes(int M, int P, int Q);
int egomi_lora_wgrad(const void* l, int64_t ldl, const void* r, int64_t ldr, float* g, int64_t ldg, int M, int P, int Q, float alpha,
                     int accumulate, int il, void* workspace, int64_t workspace_bytes, int dtype, egomi_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * A14  trajectory <-> token ids for whole batches, displacement metrics (integer contracts bit-exact).
 * replaces models/pointllm/utils/utils.py:13-21 (discretize_action / token_to_action), :47-104
 * (str_to_float, rt2 6-DoF: split on <tsep>, first run of six <p*> tokens per segment, unmatched
 * segments repeat the previous step), the sequence layout of models/pointllm/dataset.py:150-194 and
 * models/utils/metrics.py:7-55 (ADE/FDE, documented [T,D] form, float64).
 * bins: float64 [num_bins] = numpy.linspace(-1, 1, num_bins), computed by the caller (device memory).
 *   tokenize  : traj f32 [B,Tmax,6], steps i32 [B] (NULL = Tmax) -> ids i64 [B,L] =
 *               <ts> (p*6 <tsep>) x steps <te> <eos> pad..., mask u8 [B,L]; err[b]=1 if L is too short
 *               (sequence truncated to whole steps).  bin = clamp(digitize(v)-1, 0, num_bins-1).
 *   detokenize: ids i64 [B,L] (cut at the first eos) -> out f32 [B,Tmax,6] bin values, n_steps i32 [B]
 *   metrics   : gen/gt f32 [B,Tmax,D] with lengths (NULL = Tmax; a length above Tmax counts as Tmax, as in every trajectory entry
 *               point: nothing past a buffer is read) -> ade, fde float64 [B]; NaN, NaN when either length is <= 0
 */
int egomi_traj_tokenize(const float* traj, const int32_t* steps, int B, int Tmax, const double* bins, int num_bins, int64_t p0,
                        int64_t ts, int64_t tsep, int64_t te, int64_t eos, int64_t pad, int L, int64_t* ids, uint8_t* mask,
                        int32_t* err, egomi_stream_t stream);
int egomi_traj_detokenize(const int64_t* ids, int B, int L, const double* bins, int num_bins, int64_t p0, int64_t tsep, int64_t eos,
                          int Tmax, float* out, int32_t* n_steps, egomi_stream_t stream);
/* detokenize_soft: `detokenize`'s scan on the same ids (cut at the first eos, split on <tsep>, first run of six bin ids per segment,
 *              copy-forward), gathering egomi_bin_stats' per-token results instead of bin centres.  bin_mean, bin_std f32 [B, >= L] (row
 *              stride ld_stat; column j describes ids[:, j]), bin_mass likewise or NULL.  A step parsed from ids hit .. hit+5:
 *              mean[b,n,c] = bin_mean[b,hit+c], std[b,n,c] = bin_std[b,hit+c], mass[b,n] = min over c of bin_mass[b,hit+c] (a NaN among
 *              them gives NaN); a copied step repeats all three.  mean, std f32 [B,Tmax,6], mass f32 [B,Tmax] (NULL exactly when bin_mass
 *              is), n_steps i32 [B] = `detokenize`'s on the same ids; steps >= n_steps are not written.  BADARG (NULL ids / bin_mean /
 *              bin_std / mean / std / n_steps, bin_mass without mass or the reverse), SHAPE (a size <= 0, num_bins <= 1, ld_stat < L). */
int egomi_traj_detokenize_soft(const int64_t* ids, int B, int L, int num_bins, int64_t p0, int64_t tsep, int64_t eos, const float* bin_mean,
                               const float* bin_std, const float* bin_mass, int64_t ld_stat, int Tmax, float* mean, float* std,
                               float* mass, int32_t* n_steps, egomi_stream_t stream);
int egomi_traj_metrics(const float* gen, const int32_t* n_gen, const float* gt, const int32_t* n_gt, int B, int Tmax, int D, double* ade,
                       double* fde, egomi_stream_t stream);
/* metrics_min: best-of-K (minADE_K / minFDE_K; the reference's run_validation, train.py:207-264, scores one draw per clip with
 *              models/utils/metrics.py:7-55).  gen f32 [B,K,Tmax,D], n_gen i32 [B,K] (NULL = Tmax), gt f32 [B,Tmax,D], n_gt i32 [B] (NULL = Tmax);
 *              lengths above Tmax count as Tmax -> min_ade, min_fde float64 [B], best i32 [B].  Every sample is scored as `metrics` scores it; samples with n_gen <= 0 take no
 *              part; best = arg-min ADE (lowest index on ties); min_fde is the minimum over the samples, not the FDE of `best`; no sample
 *              left (or n_gt <= 0): NaN, NaN, -1. */
int egomi_traj_metrics_min(const float* gen, const int32_t* n_gen, const float* gt, const int32_t* n_gt, int B, int K, int Tmax, int D,
                           double* min_ade, double* min_fde, int32_t* best, egomi_stream_t stream);
/* medoid     : the most central of K samples, a choice that needs neither the ground truth nor model scores (the displacement of
 *              models/utils/metrics.py:38-55 between two samples).  gen f32 [B,K,Tmax,D], n_gen i32 [B,K] (NULL = Tmax; values above Tmax
 *              count as Tmax); sample j is valid when n_gen > 0.  d(j,i) = mean over t < max(n_j, n_i) of ||g_j[min(t,n_j-1)] -
 *              g_i[min(t,n_i-1)]||_2 over all D dims (each padded with its own last step, as `metrics` pads).  cost[b,j] float64 = mean of
 *              d(j,i) over the valid i != j, summed in index order; one valid sample: 0; invalid j: NaN.  pick[b] i32 = arg-min of cost
 *              over the valid samples (lowest index on ties), none: -1.  BADARG (NULL gen / cost / pick), SHAPE (a size <= 0),
 *              UNSUPPORTED (K > 1024). */
int egomi_traj_medoid(const float* gen, const int32_t* n_gen, int B, int K, int Tmax, int D, double* cost, int32_t* pick,
                      egomi_stream_t stream);
/* modes      : M mutually different of K samples, each with a probability (csrc/modes.hip): the short list between all K (`metrics_min`)
 *              and one pick (`medoid`, seq_rank).  gen f32 [B,K,Tmax,D], n_gen i32 [B,K] (NULL = Tmax; values above Tmax count as Tmax),
 *              score f32 [B,K] or NULL, K <= 64, M <= 64 (M > K is legal).  Sample j is valid when n_gen > 0; an invalid sample is never a
 *              mode and has no place in the order.  Values of gen are expected finite.
 *   dist     float64 [B,K,K], may be NULL: d(j,i) of `medoid`, each unordered pair computed once and stored to both halves (bit-symmetric);
 *              diagonal of a valid sample 0.0; NaN wherever j or i is invalid.
 *   order    with score: descending score, ties -> lower index, a NaN score ranks as -inf, -inf rows last in index order (seq_rank's rules).
 *              score == NULL: ascending centrality c_j = mean of d(j,i) over the valid i != j, summed in index order and divided once
 *              (`medoid`'s cost, the same expression in the same order; 0 for a single valid sample), ties -> lower index: with M = 1 the
 *              pick is `medoid`'s pick.  That equality of picks is the contract; c_j is not returned, and its bits are not promised to be
 *              those of `medoid`'s cost (the two kernels are separate compilations of the expression).
 *   NMS      walk the order; a sample becomes the next mode when d(j,m) > radius for every mode m picked so far; stop at M modes or at the
 *              end of the order.  n_nms[b] i32 = modes picked this way.
 *   fill     while fewer than M: among the valid unpicked samples the one whose minimum distance to the picked modes is largest (ties ->
 *              lower index); stop when that distance is <= 0 (what is left are exact duplicates) or no sample is left.  n_modes[b] i32 =
 *              the total; modes[b, :n_modes] i32 = sample indices in pick order, the rest -1.
 *   assign   i32 [B,K]: the slot m in 0 .. n_modes-1 of the nearest mode (ties -> lower slot; a mode is assigned to itself), invalid: -1.
 *   conf     float64 [B,M]: (double)count(assign == m) / (double)n_valid, the Monte-Carlo mass of the mode under the distribution the
 *              samples were drawn from; unused slots 0.0.  A clip without a valid sample: all -1 / 0.0, n_modes = n_nms = 0.
 *              BADARG (NULL gen / modes / conf / assign / n_modes / n_nms; NaN or negative radius -- radius = 0 is legal and suppresses
 *              exact duplicates only), SHAPE (B, K, Tmax, D or M <= 0), UNSUPPORTED (K > 64 or M > 64).  No atomics; the order of every
 *              sum depends on (K, Tmax, D, n_gen) only: a replay is bit-equal. */
int egomi_traj_modes(const float* gen, const int32_t* n_gen, const float* score, int B, int K, int Tmax, int D, int M, double radius,
                     double* dist, int32_t* modes, double* conf, int32_t* assign, int32_t* n_modes, int32_t* n_nms,
                     egomi_stream_t stream);
/* metrics_full: the five measures of models/utils/metrics.py per sample, one launch (csrc/traj_full.hip).  gen f32 [B,K,Tmax,D], n_gen i32 [B,K]
 *              (NULL = Tmax), gt f32 [B,Tmax,D], n_gt i32 [B] (NULL = Tmax); lengths above Tmax count as Tmax; nothing of a row beyond its
 *              length is read.  out float64 [B,K,5] = ADE, FDE, IDE, GD, DTW; all five NaN when n_gen <= 0 or n_gt <= 0.
 *   ADE, FDE   `metrics` on the same row, bit for bit (gen padded with its last step / cut to n_gt).
 *   IDE        ||gt[0] - gen[0]||_2 over all D dims (metrics.py:29-36).
 *   GD         metrics.py:61-87 on columns rot0 .. rot0+2 as rotation vectors, gen padded / cut as for ADE: the sum over t < n_gt, in index
 *              order, of 2 acos(clip(<q(gen_t), q(gt_t)>, -1, 1)), divided by n_gt; q(r) = (s r, cos(|r|/2)), s = sin(|r|/2) / |r| for
 *              |r| > 1e-3, else 0.5 - |r|^2/48 + |r|^4/3840 (scipy's from_rotvec).  The dot product is used as it is, not its absolute
 *              value.  rot0 < 0 or rot0 + 3 > D: NaN for every row (position-only input).
 *   DTW        metrics.py:57-59 as the exact dynamic programme on x = gen[:n_gen], y = gt[:n_gt], no padding and no cut: c(i,k) =
 *              ||x_i - y_k||_2 over all D dims, Dp(i,k) = c(i,k) + min(Dp(i-1,k), Dp(i,k-1), Dp(i-1,k-1)), Dp(0,0) = c(0,0); the value is
 *              Dp(n_gen-1, n_gt-1), not normalised by the path length.  (The reference calls fastdtw(radius=1): exact while either
 *              sequence has fewer than 3 steps, otherwise an upper bound of this value.)
 *   mins, args float64 / i32 [B,5], NULL together: per column the minimum over the clip's samples whose value is not NaN and that sample's
 *              index (lowest index on ties); no such sample: NaN, -1.  Columns 0, 1 are `metrics_min`'s min_ade, min_fde bit for bit,
 *              args[b,0] its best.
 *              BADARG (NULL gen / gt / out, one of mins / args NULL), SHAPE (B <= 0, K < 1, Tmax outside 1 .. 256, D outside 1 .. 64).
 *              No atomics, no state between launches: a replay is bit-equal, and a row's bits depend on neither K, its slot, B nor the
 *              lengths of its neighbours. */
int egomi_traj_metrics_full(const float* gen, const int32_t* n_gen, const float* gt, const int32_t* n_gt, int B, int K, int Tmax, int D, int rot0,
                            double* out, double* mins, int32_t* args, egomi_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Trainable point backbone (--unfreeze_pc_encoder, models/pointllm/model_arch.py:33-36): the backward
 * and train-mode pieces of pointbert/dvae.py:189-221 (Conv1d / BatchNorm1d / ReLU / max) and
 * pointbert/point_encoder.py:58-76,142 (LayerNorm, DropPath residual).
 *   layernorm_bwd : dx = dx_add + LN'(dy); dw, db (fp32 [cols], caller-zeroed, may be NULL) accumulate
 *   bn_train_fwd  : y = relu?(BatchNorm1d(x)) with BATCH statistics over the R rows (biased variance),
 *                   running stats updated with `momentum` (unbiased variance), stats = fp32 [4*C]
 *                   scratch/saved block {sum, sumsq (both of x - x[0,:]: scratch), mean, rstd (saved)}
 *   bn_train_bwd  : dx, dgamma, dbeta (fp32 [C], written by the call) from dy, x, y and the saved stats
 *   group_argmax  : x [BG,M,C] -> max over M and its first arg-max;  group_max_bwd scatters dout back
 *   smallk_wgrad  : dW[n,k] (fp32, caller-zeroed/accumulating) += sum_r dy[r,n]*x[r,k], K <= 8
 *   group_sum     : out[bg,c] = sum_m x[(bg*M+m)*ldx + c]  (backward of the expanded group-global feature)
 *   rowscale_add  : out[r,:] = resid[r,:] + scale[r / rows_per_sample] * branch[r,:]   (DropPath)
 * Column reductions (dw / db, the batch statistics, dgamma / dbeta, dW) are two-stage and ORDERED — one partial row per block in the caller's
 * fp32 scratch `partials`, added in block order by a second kernel; no atomics, the same bits every run (the batch statistics feed the
 * forward output, so this makes the train-mode backbone's forward replayable too).  `partial_floats` must be at least
 *   layernorm_bwd (dw or db given): min(ceil(rows / 4), 512) * 2 * cols        bn_train_fwd / bn_train_bwd: ceil(R / 256) * 2 * C
 *   smallk_wgrad: ceil(R / 512) * N * K
 * (EGOMI_E_BADARG otherwise); cols <= 2048 for layernorm_bwd.
 */
int egomi_layernorm_bwd(const void* dy, const void* x, const void* w, void* dx, const void* dx_add, float* dw, float* db,
                        int rows, int cols, float eps, float* partials, int64_t partial_floats, int dtype, egomi_stream_t stream);
int egomi_bn_train_fwd(const void* x, int64_t R, int C, const void* gamma, const void* beta, float eps, int relu, void* y,
                       float* stats, void* running_mean, void* running_var, float momentum, float* partials, int64_t partial_floats, int dtype,
                       egomi_stream_t stream);
int egomi_bn_train_bwd(const void* dy, const void* x, const void* y, int64_t R, int C, const float* stats, const void* gamma, int relu,
                       float* dgamma, float* dbeta, void* dx, float* partials, int64_t partial_floats, int dtype, egomi_stream_t stream);
int egomi_group_argmax(const void* x, int BG, int M, int C, void* out, int32_t* idx, int dtype, egomi_stream_t stream);
int egomi_group_max_bwd(const void* dout, const int32_t* idx, int BG, int M, int C, void* dx, int64_t ldx, int accumulate, int dtype,
                        egomi_stream_t stream);
int egomi_smallk_wgrad(const void* dy, const void* x, int x_dtype, int64_t R, int N, int K, float* dW, float* partials, int64_t partial_floats, int dtype,
                       egomi_stream_t stream);
int egomi_group_sum(const void* x, int BG, int M, int C, int64_t ldx, void* out, int dtype, egomi_stream_t stream);
int egomi_rowscale_add(const void* resid, const void* branch, const float* scale, int64_t rows, int cols, int rows_per_sample, void* out,
                       int dtype, egomi_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Row / elementwise kernels (HBM-bound).  `dtype` is the activation/parameter dtype T.
 */
/* LayerNorm forward with optional fused pre-add: s = x (+ add); y = (s-mean)*rstd*w + b; sum_out = s
 * replaces nn.LayerNorm in pointbert/point_encoder.py:60,63,142 and the `x + pos` of :95-98 */
int egomi_layernorm_fwd(const void* x, const void* add, const void* w, const void* b, void* sum_out, void* y,
                        int rows, int cols, float eps, int dtype, egomi_stream_t stream);

/* RMSNorm.  replaces HF LlamaRMSNorm, transformers/models/llama/modeling_llama.py:53-67 (A11).
 * fwd: y = w * T(x * rsqrt(mean(x^2)+eps)); rstd [rows] saved when non-NULL.  cols % 8 == 0.
 * bwd: dx = dx_add + rstd*(w*dy - x_hat*mean(w*dy*x_hat)); dw [cols] fp32 += sum_rows dy*x_hat
 *      (dx_add, dw may be NULL).  cols <= 8192. */
int egomi_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd, int rows, int cols, float eps, int dtype,
                      egomi_stream_t stream);
int egomi_rmsnorm_bwd(const void* dy, const void* x, const void* w, const float* rstd, void* dx, const void* dx_add,
                      float* dw, int rows, int cols, int dtype, egomi_stream_t stream);
/* egomi_rmsnorm_bwd on COMPACT rows: dy, x, rstd, dx, dx_add hold only the last `win` rows of every sequence of `seq` rows (rows = sequences * win).
 * dw is summed in the order of the full-layout call whose other rows have dy = 0, so it has that call's bits. */
int egomi_rmsnorm_bwd_rows(const void* dy, const void* x, const void* w, const float* rstd, void* dx, const void* dx_add,
                           float* dw, int rows, int cols, int seq, int win, int dtype, egomi_stream_t stream);
/* Tail forms: rows >= row0 of the input (x resp. dy) are still the `slices` fp32 K-slice slabs [slices][rows - row0][cols] an
 * EGOMI_EPI_SLABS product left (egomi_gemm_tail_plan); they are summed in slice order (+ residual rows for the forward form),
 * rounded, WRITTEN to x / dy, and normalised in the same pass — bit-identical to the combine pass followed by
 * egomi_rmsnorm_fwd / egomi_rmsnorm_bwd.  row0 == rows: no pending rows (then exactly the plain kernels' arithmetic). */
int egomi_rmsnorm_fwd_tail(void* x, const void* w, void* y, float* rstd, int rows, int cols, float eps, int row0, const float* slabs, int slices,
                           const void* residual, int64_t ldr, int dtype, egomi_stream_t stream);
int egomi_rmsnorm_bwd_tail(void* dy, const void* x, const void* w, const float* rstd, void* dx, const void* dx_add, float* dw, int rows,
                           int cols, int row0, const float* slabs, int slices, int dtype, egomi_stream_t stream);

/* RoPE in place on x [rows, H, hd] (row stride ld elements); position of row r = pos_offset + r % S;
 * cos/sin tables fp32 [>= pos_offset+S, hd/2].  inverse=1 applies the transposed rotation (backward).
 * replaces HF rotate_half/apply_rotary_pos_emb, modeling_llama.py:130-160 (tables: :112-127) */
int egomi_rope(void* x, const float* cos_tab, const float* sin_tab, int64_t rows, int S, int pos_offset, int H, int hd,
               int64_t ld, int inverse, int dtype, egomi_stream_t stream);
/* Tail form for the stacked q|k|v product [rows, 3*H*hd]: rows >= row0 are still `slices` K-slice slabs (EGOMI_EPI_SLABS,
 * egomi_gemm_tail_plan); they are summed, rounded and written (q, k rotated; v as is); rows < row0 get egomi_rope's rotation of
 * q and k in place.  Bit-identical to the combine pass followed by egomi_rope on the first 2*H heads. */
int egomi_rope_qkv_tail(void* qkv, const float* cos_tab, const float* sin_tab, int64_t rows, int S, int pos_offset, int H, int hd, int64_t ld,
                        int row0, const float* slabs, int slices, int dtype, egomi_stream_t stream);

/* SwiGLU: out = silu(gate)*up.  replaces HF LlamaMLP.forward, modeling_llama.py:174-176.
 * gate/up [rows, cols] with row stride ld_in; out / dgate / dup row stride ld_out; dact row stride ld_act. */
int egomi_swiglu_fwd(const void* gate, const void* up, void* out, int64_t rows, int cols, int64_t ld_in, int64_t ld_out,
                     int dtype, egomi_stream_t stream);
int egomi_swiglu_bwd(const void* dact, const void* gate, const void* up, void* dgate, void* dup, int64_t rows, int cols,
                     int64_t ld_in, int64_t ld_act, int64_t ld_out, int dtype, egomi_stream_t stream);
/* The same two ops on the "interleaved-32" gate|up layout: gu / dgu are ONE [rows, 2*cols] array in which hidden unit c
 * sits at column 64*(c/32) + c%32 (gate) and 32 columns further (up).  It is what x . [Wgate;Wup]^T yields when the rows of
 * the stacked weight are interleaved in blocks of 32, which puts gate and up of the same units into the same GEMM wave
 * (egomi_gemm epilogue EGOMI_EPI_SWIGLU).  cols % 32 == 0. */
int egomi_swiglu_il_fwd(const void* gu, void* out, int64_t rows, int cols, int64_t ld_gu, int64_t ld_out, int dtype, egomi_stream_t stream);
int egomi_swiglu_il_bwd(const void* dact, const void* gu, void* dgu, int64_t rows, int cols, int64_t ld_gu, int64_t ld_act, int64_t ld_dgu,
                        int dtype, egomi_stream_t stream);

/* exact (erf) GELU and its derivative.  replaces nn.GELU in point_proj, model/pointllm.py:72-76 */
int egomi_gelu_fwd(const void* x, void* y, int64_t n, int dtype, egomi_stream_t stream);
int egomi_gelu_bwd(const void* dy, const void* x, void* dx, int64_t n, int dtype, egomi_stream_t stream);

/* Row softmax of fp32 scores [Z*Sq, Sk] (row stride ld_s) -> P (dtype, row stride ld_p).
 * key j is visible to query i iff (!causal || j <= q_offset+i) && (key_mask == NULL || key_mask[b*Sk+j]),
 * b = z / heads.  replaces pointbert/point_encoder.py:48-50 and HF eager_attention_forward,
 * modeling_llama.py:204-210.  Sk <= 2048.   bwd: dS = P*(dP - sum_j P*dP). */
int egomi_softmax_fwd(const float* scores, int64_t ld_s, const uint8_t* key_mask, int Z, int heads, int Sq, int Sk, int causal,
                      int q_offset, void* P, int64_t ld_p, int dtype, egomi_stream_t stream);
int egomi_softmax_bwd(const void* P, int64_t ld_p, const float* dP, int64_t ld_dp, void* dS, int64_t ld_ds, int64_t rows, int Sk,
                      int dtype, egomi_stream_t stream);

/* A10  point-token splice.  replaces model/pointllm.py:131-171 (mm_use_point_start_end=True).
 * splice_scan: per sample start_pos = position of the <point_start> whose span receives the features (-1: text-only sample or
 * error), cloud_idx = which of the n_clouds clouds it receives (the reference's running cur_point_idx, :135,143,156), and
 * err: 0 ok | 1 start/end count mismatch (:146) | 2 a <point_end> not at start+P+1 (:150) | 4 cloud index past the clouds given
 * (:143 IndexError).  A sample with several segments is treated as the reference treats it: only its LAST segment is spliced,
 * with the cloud the sample started at, and the cloud index advances once per segment.  scratch: B int32.
 * embed_splice_fwd: out[b,s] = feats[cloud_idx[b], s-start-1] if start < s <= start+P else W[ids[b,s]]
 * (embedding lookup :107 + torch.cat splice :155).  bwd: dW (fp32 [V,d]) += rows outside the span,
 * dfeats[cloud_idx[b]] = rows inside it (rows of clouds no sample received are not written: zero them first).
 * feats/start_pos/dW/dfeats may be NULL; cloud_idx NULL = cloud b for sample b. */
int egomi_splice_scan(const int64_t* ids, int B, int S, int64_t patch_id, int64_t start_id, int64_t end_id, int P, int n_clouds,
                      int32_t* start_pos, int32_t* err, int32_t* cloud_idx, int32_t* scratch, egomi_stream_t stream);
int egomi_embed_splice_fwd(const int64_t* ids, const void* W, const void* feats, const int32_t* start_pos, const int32_t* cloud_idx,
                           int B, int S, int d, int P, int V, void* out, int dtype, egomi_stream_t stream);
int egomi_embed_splice_bwd(const void* dout, const int64_t* ids, const int32_t* start_pos, const int32_t* cloud_idx, int B, int S, int d,
                           int P, int V, float* dW, void* dfeats, int dtype, egomi_stream_t stream);

/* A12  cross-entropy with ignore_index, mean over kept rows.  replaces F.cross_entropy at
 * models/pointllm/train.py:174-181.  count must be zeroed, then ce_count, then ce_fwd_bwd:
 * row_loss[R] (fp32 scratch of the caller) = -log p[target] per row (0 for ignored rows), loss_sum (fp32, zeroed by caller) += their sum
 * in a fixed order (no atomics: the same bits every run); dlogits (may alias logits, may be NULL) = (softmax - onehot) * grad_scale / count. */
int egomi_ce_count(const int64_t* targets, int64_t n, int64_t ignore, int32_t* count, egomi_stream_t stream);
int egomi_ce_fwd_bwd(const void* logits, int64_t ld, const int64_t* targets, int R, int V, int64_t ignore, const int32_t* count,
                     float* loss_sum, float* row_loss, void* dlogits, int64_t ldd, float grad_scale, int dtype, egomi_stream_t stream);

/* A12 (soft)  the same loss against a bin-aware target (label-distribution learning for the binned regression head); the reference's
 * F.cross_entropy at models/pointllm/train.py:174-181 is its one-hot case.  count as above (zeroed, then ce_count).  A kept row whose target t
 * is one of the nb contiguous bin ids p0 .. p0 + nb - 1 is scored against q[p0 + j] = w_j / Z, w_j = exp(-(j - i)^2 / (2 sigma^2)) for
 * max(0, i - radius) <= j <= min(nb - 1, i + radius), i = t - p0, Z = sum w_j (float64, j ascending): truncation renormalises, no mass leaves
 * the bin window, nb = 1 is the one-hot.  Every other kept target keeps the one-hot; ignored rows (t == ignore, t < 0, t >= V) give 0 and a
 * zero gradient row.  row_loss[R] = sum_j q_j (lse - x_j), row_nll[R] = lse - x_t (the hard loss, comparable with ce_fwd_bwd's); loss_sum and
 * nll_sum (fp32, zeroed by caller) += their sums in a fixed order (no atomics: the same bits every run).  dlogits (may alias logits, may be
 * NULL) = (softmax - q) * grad_scale / count; nothing outside [row, row + V) is written.  sigma in bins, 0 < sigma <= 16; 1 <= radius <= 32. */
int egomi_ce_soft_fwd_bwd(const void* logits, int64_t ld, const int64_t* targets, int R, int V, int64_t ignore, const int32_t* count,
                          int p0, int nb, float sigma, int radius, float* loss_sum, float* nll_sum, float* row_loss, float* row_nll,
                          void* dlogits, int64_t ldd, float grad_scale, int dtype, egomi_stream_t stream);

/* AdamW step (torch.optim.AdamW semantics; reference optimizer models/pointllm/train.py:107-111).
 * fp32 master/moments/grad; model_copy (copy_dtype, may be NULL) receives the updated value. */
int egomi_adamw(float* master, void* model_copy, const float* grad, float* m, float* v, int64_t n, float lr, float beta1,
                float beta2, float eps, float weight_decay, int step, float grad_scale, int copy_dtype, egomi_stream_t stream);
/* The same step with the gradient given in bf16: the rank-summed wire buffer of the data-parallel exchange read in place (what DeepSpeed's
 * bf16 engine does after its reduce: fp32 master / moments updated from the reduced low-precision gradient, train.py:92-104,184). */
int egomi_adamw_g16(float* master, void* model_copy, const void* grad_bf16, float* m, float* v, int64_t n, float lr, float beta1,
                    float beta2, float eps, float weight_decay, int step, float grad_scale, int copy_dtype, egomi_stream_t stream);
/* Both steps with grad_scale read from device memory (grad_scale_dev, one fp32: egomi_clip_scale's out[2]) instead of passed by value.
 * Same element arithmetic and the same 16-B / scalar split: a device value equal to the host value gives master, m, v and model_copy the
 * bits of the two entry points above. */
int egomi_adamw_ds(float* master, void* model_copy, const float* grad, float* m, float* v, int64_t n, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int step, const float* grad_scale_dev, int copy_dtype, egomi_stream_t stream);
int egomi_adamw_g16_ds(float* master, void* model_copy, const void* grad_bf16, float* m, float* v, int64_t n, float lr, float beta1,
                       float beta2, float eps, float weight_decay, int step, const float* grad_scale_dev, int copy_dtype,
                       egomi_stream_t stream);

/* Gradient-norm clipping (torch.nn.utils.clip_grad_norm_ semantics; the reference does not clip — HF Trainer max_grad_norm and
 * DeepSpeed gradient_clipping are what users of the added training modes expect).
 *
 * grad_sumsq: the sum of squares of n_seg gradient tensors ("segments") in one call of two launches, whatever n_seg.
 *   seg_addr  i64 [n_seg]  device address of each segment (contiguous elements)
 *   seg_numel i64 [n_seg]  element count of each; each must be > 0 (device data: the call cannot check it; a count <= 0 contributes 0)
 *   seg_dtype i32 [n_seg]  EGOMI_F32 / EGOMI_BF16 per segment, or NULL: every segment has `dtype` (every table outside data parallelism is
 *                          fp32 throughout).  `dtype` is not read when a table is given, but must be one of the two either way
 *                          (UNSUPPORTED); the table is device data, which the call cannot check: an entry that is neither makes that
 *                          segment's sum, and the total, NaN, and nothing is read through its address
 *   n_chunks               sum over the segments of ceil(numel / C), C = egomi_grad_sumsq_chunk() elements (or more: surplus workgroups do
 *                          nothing).  The caller knows the counts it wrote into the table.  Fewer than the table needs: the segments
 *                          past it and the total report NaN; nothing is read or written out of bounds
 *   seg_sumsq f64 [n_seg], total_sumsq f64 [1] (both written, not accumulated);  workspace: egomi_grad_sumsq_workspace_bytes, 8-B aligned
 * Stage 1: one workgroup per chunk of C elements of one segment, 16-B loads, every element widened to float64, squared (exact) and
 * added in float64 in a fixed order — fp32 squares overflow above 1.8e19 and vanish below 1e-19; float64 does neither, and the pass is
 * HBM-bound whatever the arithmetic — one float64 partial per chunk.  Stage 2: one workgroup adds each segment's partials, then the
 * segments, in a fixed order (lane-strided in ascending index, then a fixed tree).  No atomics of any kind.
 * Contract: a segment's seg_sumsq bits depend only on its element count, dtype and values — not on its position in the table, its
 * neighbours or n_seg, not on the alignment of its address (a segment that is not 16-B aligned takes 4-B / 2-B loads with the same
 * element-to-lane mapping), not on the grid (n_chunks) and not on which run it is.  total_sumsq's bits depend on the seg_sumsq values in
 * table order.  All index arithmetic is 64-bit.
 * Errors: BADARG for a NULL table, output or workspace; SHAPE for n_seg <= 0, n_chunks < n_seg or > 2^31-1, or a workspace that is too
 * small or not 8-B aligned; UNSUPPORTED for `dtype`.
 *
 * clip_scale: one thread, float64.  out f32 [3]:
 *   out[0] = total_norm = grad_scale * sqrt(total_sumsq)   (the norm of the gradient the update applies, 1/world and 1/accum folded in)
 *   out[1] = coef = min(1, max_norm / (total_norm + 1e-6)) (clip_grad_norm_ with its 1e-6; a NaN norm gives a NaN coefficient)
 *   out[2] = grad_scale itself, bit for bit, when coef >= 1; else (float)((double)grad_scale * coef) — what the _ds steps above read
 * stats f64 [5], accumulated in place (the caller zeroes it for a fresh window): steps seen, steps clipped (finite norm, coef < 1),
 * steps whose fp32 total_norm is not finite, the sum of the finite norms, their maximum.
 * max_norm = +inf is legal ("measure only": coef is 1 whenever the norm is finite); max_norm <= 0 or NaN is BADARG. */
int64_t egomi_grad_sumsq_chunk(void);
size_t egomi_grad_sumsq_workspace_bytes(int n_seg, int64_t n_chunks);
int egomi_grad_sumsq(const int64_t* seg_addr, const int64_t* seg_numel, const int32_t* seg_dtype, int dtype, int n_seg, int64_t n_chunks,
                     double* seg_sumsq, double* total_sumsq, void* workspace, size_t workspace_bytes, egomi_stream_t stream);
int egomi_clip_scale(const double* total_sumsq, float grad_scale, float max_norm, float* out, double* stats, egomi_stream_t stream);

/* layout helpers: out[c, r] = in[r, c] for r < R, zero for R <= r < ldo; cast; add */
int egomi_transpose(const void* in, int R, int C, int64_t ldi, void* out, int64_t ldo, int dtype, egomi_stream_t stream);
int egomi_cast(const void* in, int in_dtype, void* out, int out_dtype, int64_t n, egomi_stream_t stream);
int egomi_add(const void* a, const void* b, void* out, int64_t n, int dtype, egomi_stream_t stream);
/* Gradient exchange of the data-parallel step (replaces DeepSpeed's bucketed gradient reduction behind
 * model_engine.backward/step, train.py:92-125,183-184): the reduce half of a direct reduce-scatter.  in [W, c] holds the
 * chunk each of the W ranks sent to this one (all-to-all over xGMI, bf16 on the wire); out [c] = their sum accumulated in
 * fp32 in rank order.  c % 8 == 0, pointers 16-B aligned.  (in,out) dtypes: (bf16,bf16) (bf16,f32) (f32,f32). */
int egomi_rank_sum(const void* in, int in_dtype, int W, int64_t c, void* out, int out_dtype, egomi_stream_t stream);
/* out[c] (fp32, caller-initialised) += sum_r x[r,c]: bias gradients (backward of nn.Linear bias, model/pointllm.py:67-81) */
int egomi_colsum(const void* x, int64_t R, int C, int64_t ld, float* out, int dtype, egomi_stream_t stream);

/* A6 helpers.  group_max: x [BG, M, C] -> out [BG, C] (concat=0) or [BG*M, 2C] = [group max | x]
 * (concat=1).  replaces torch.max / cat / expand at pointbert/dvae.py:216-219.
 * linear_smallk: y = act(x.w^T + b) for K <= 8 (x may be fp32): pos_embed.0 (point_encoder.py:128)
 * and the first 1x1 conv (dvae.py:194). */
int egomi_group_max(const void* x, int BG, int M, int C, void* out, int concat, int dtype, egomi_stream_t stream);
int egomi_linear_smallk(const void* x, int x_dtype, const void* w, const void* b, void* y, int64_t R, int N, int K, int act,
                        int dtype, egomi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EGOMI_H */
